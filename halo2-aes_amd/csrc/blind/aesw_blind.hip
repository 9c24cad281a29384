// blind/aesw_blind.hip -- libaesw_blind.so (include/aesw_blind.h): the blinding rows of a column and the commitment of a blinded tail,
// on the device.  The rule -- the keyed hash of (seed, domain, column, row), the wide reduction, the fixed
// double-and-add of a term -- is aesw_blind.h's over aesw_transcript.h's Blake2b and aesw_msm.h's group; nothing of it is restated
// here.  What is here:
//   * blind_cells_kernel<NT>: a lane per cell.  The lane compresses the key block and then its own message block: two compressions
//     a cell.  The key block's is the same in every lane, and no kernel of its own derives it once: that would need a buffer
//     between two launches, and a call allocates nothing.  One kernel serves aesw_blind_rows_device (the cells where the columns
//     lie) and aesw_blind_tail_device (compactly): they differ in the stride of a column and in where its first cell goes;
//   * blind_commit_tail_kernel: ONE wave per column and one lane per tail row.  A lane takes its cell times its basis point by
//     blind_term, 254 doublings and mixed additions in lockstep with a select on the bit; the lanes without a row hold the
//     identity.  The 64 points are summed by six xor-shuffle steps of the complete addition, the old commitment is mixed in once,
//     one fq_inv, and lane 0 stores the 64 bytes.
// No atomic of any kind, no LDS, no scratch: every index into registers is a constant.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_blind.h"
#include "../aesw_blind.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"

namespace aesw_blind {
using namespace aesw;

constexpr int THREADS = 256;
static_assert(MSM_LANES == LANES && BLIND_MAX_TAIL == LANES && AESW_BLIND_MAX_TAIL == BLIND_MAX_TAIL && AESW_BLIND_SEED_BYTES == BLIND_SEED_BYTES,
              "the rules count the lanes, the tail and the seed as the device and the header do");

// ---- the cells ----------------------------------------------------------------------------------------------------------------------

struct CellsParams {
    const uint64_t *seed;  // four words
    u32x4 *out;
    uint64_t first_row, rows;       // the rows hashed: first_row ... first_row + rows - 1
    uint64_t stride, first_stored;  // column j's cell of row first_row + i goes to cell j * stride + first_stored + i of out
    uint64_t domain, first_column;
};

// grid: x = 256 rows of the tail, y = the column
template <int NT>
__global__ void __launch_bounds__(THREADS) blind_cells_kernel(const CellsParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= p.rows) return;
    const uint64_t seed[4] = {p.seed[0], p.seed[1], p.seed[2], p.seed[3]};
    const Fr cell = blind_cell(blind_key(seed), p.domain, p.first_column + blockIdx.y, p.first_row + i);
    store_cell<NT>(cell_at(p.out, (uint64_t)blockIdx.y * p.stride + p.first_stored + i), cell);
}

// ---- the tail commitment ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ Fq load_fq(const u32x4 *p) {
    const u32x4 lo = p[0], hi = p[1];
    return Fq{{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
}
__device__ __forceinline__ void store_fq(u32x4 *p, const Fq &v) {
    p[0] = u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
    p[1] = u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
}
__device__ __forceinline__ G1Affine load_affine(const u32x4 *base, uint64_t i) { return G1Affine{load_fq(base + i * 4), load_fq(base + i * 4 + 2)}; }
__device__ __forceinline__ Fq shfl_xor_fq(const Fq &v, int o) {
    Fq r = FQ_ZERO;
#pragma unroll
    for (int i = 0; i < FQ_LIMBS; ++i) r.l[i] = __shfl_xor(v.l[i], o, LANES);
    return r;
}
__device__ __forceinline__ G1 shfl_xor_point(const G1 &p, int o) { return G1{shfl_xor_fq(p.x, o), shfl_xor_fq(p.y, o), shfl_xor_fq(p.z, o)}; }

// grid: x = the column; one wave.  tail: 1 ... 64 rows.
__global__ void __launch_bounds__(LANES) blind_commit_tail_kernel(const u32x4 *__restrict__ tail_cells, const u32x4 *__restrict__ basis, u32x4 *commit, uint64_t first_row,
                                                                  uint32_t tail) {
    const uint32_t lane = threadIdx.x, column = blockIdx.x;
    Fr cell = FR_ZERO;
    G1Affine point{FQ_ZERO, FQ_ZERO};  // a lane without a row: zero times the identity
    if (lane < tail) {
        cell = load_cell(cell_at(tail_cells, (uint64_t)column * tail + lane));
        point = load_affine(basis, first_row + lane);
    }
    G1 acc = blind_term(cell, point);
#pragma unroll 1
    for (int o = LANES / 2; o; o >>= 1) acc = msm_add(acc, shfl_xor_point(acc, o));
    acc = msm_add_mixed(acc, load_affine(commit, column));  // every lane reads the old commitment before lane 0 stores the new one: one wave
    const G1Affine sum = msm_to_affine(acc);
    if (lane == 0) {
        store_fq(commit + (uint64_t)column * 4, sum.x);
        store_fq(commit + (uint64_t)column * 4 + 2, sum.y);
    }
}

// ---- the checks -----------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }

// both fills: `compact` stores the tail alone
int cells(aesw_ctx *ctx, const char *call, const char *out_name, bool compact, uint32_t k, uint32_t n_cols, uint64_t first_row, uint64_t domain, uint64_t first_column,
          const uint8_t *d_seed, uint8_t *d_out, void *stream) {
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!blind_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (!blind_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 65535");
    if (!blind_first_row_ok(k, first_row)) return refuse(ctx, call, "first_row must be below 2^k");
    if (bad_pointer(d_seed)) return refuse(ctx, call, "d_seed must be there and 16-byte aligned");
    if (bad_pointer(d_out)) return refuse(ctx, call, (std::string(out_name) + " must be there and 16-byte aligned").c_str());
    const uint64_t rows = blind_tail_rows(k, first_row), stride = compact ? rows : (uint64_t)1 << k;
    if (overlap(d_out, (uint64_t)n_cols * stride * sizeof(Fr), d_seed, BLIND_SEED_BYTES)) return refuse(ctx, call, (std::string(out_name) + " must not overlap d_seed").c_str());
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    CellsParams p{};
    p.seed = reinterpret_cast<const uint64_t *>(d_seed);
    p.out = reinterpret_cast<u32x4 *>(d_out);
    p.first_row = first_row;
    p.rows = rows;
    p.stride = stride;
    p.first_stored = compact ? 0 : first_row;
    p.domain = domain;
    p.first_column = first_column;
    const dim3 grid((uint32_t)((rows + THREADS - 1) / THREADS), n_cols);  // at most 2^20 by 65535
    with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(blind_cells_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), p); });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // namespace aesw_blind

extern "C" {

uint64_t aesw_blind_tail_rows(uint32_t k, uint64_t first_row) { return aesw::blind_tail_rows(k, first_row); }

uint32_t aesw_blind_max_tail(void) { return aesw::BLIND_MAX_TAIL; }

int aesw_blind_rows_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, uint64_t domain, uint64_t first_column, const uint8_t *d_seed, uint8_t *d_cells,
                           void *stream) {
    return aesw_blind::cells(ctx, "aesw_blind_rows_device", "d_cells", false, k, n_cols, first_row, domain, first_column, d_seed, d_cells, stream);
}

int aesw_blind_tail_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, uint64_t domain, uint64_t first_column, const uint8_t *d_seed, uint8_t *d_tail,
                           void *stream) {
    return aesw_blind::cells(ctx, "aesw_blind_tail_device", "d_tail", true, k, n_cols, first_row, domain, first_column, d_seed, d_tail, stream);
}

int aesw_blind_commit_tail_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, const uint8_t *d_tail, const uint8_t *d_basis, uint8_t *d_commit,
                                  void *stream) {
    using namespace aesw_blind;
    const char *const call = "aesw_blind_commit_tail_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!blind_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (!blind_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 65535");
    if (!blind_first_row_ok(k, first_row)) return refuse(ctx, call, "first_row must be below 2^k");
    if (!blind_commit_tail_ok(k, first_row)) return refuse(ctx, call, "the tail, 2^k - first_row rows, must be at most 64");
    if (bad_pointer(d_tail)) return refuse(ctx, call, "d_tail must be there and 16-byte aligned");
    if (bad_pointer(d_basis)) return refuse(ctx, call, "d_basis must be there and 16-byte aligned");
    if (bad_pointer(d_commit)) return refuse(ctx, call, "d_commit must be there and 16-byte aligned");
    const uint32_t tail = (uint32_t)blind_tail_rows(k, first_row);
    const uint64_t commit_bytes = (uint64_t)n_cols * sizeof(G1Affine);
    if (overlap(d_commit, commit_bytes, d_tail, (uint64_t)n_cols * tail * sizeof(Fr)) || overlap(d_commit, commit_bytes, d_basis, sizeof(G1Affine) << k))
        return refuse(ctx, call, "d_commit must not overlap d_tail or d_basis");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(blind_commit_tail_kernel, dim3(n_cols), dim3(LANES), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const u32x4 *>(d_tail),
                       reinterpret_cast<const u32x4 *>(d_basis), reinterpret_cast<u32x4 *>(d_commit), first_row, tail);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
