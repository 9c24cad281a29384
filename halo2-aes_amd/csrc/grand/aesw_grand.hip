// grand/aesw_grand.hip -- libaesw_grand.so (include/aesw_grand.h): the grand product Z of every lookup argument.
// The field is aesw_fr.h's and the rules -- what an index reads, what a row multiplies Z by, Montgomery's batch inversion, how
// an argument's rows are cut into chunks, the workspace -- are aesw_grand.h's; nothing of either is restated here.  What is here:
//   * grand_invert_kernel: a lane inverts GRAND_BATCH consecutive rows of one (plane, table) with one fr_inv;
//   * grand_invert_report_kernel: one workgroup counts the zero sums (the call has no workspace to fold parts through);
//   * grand_chunk_kernel: a workgroup multiplies the factors of its chunk of one argument into one cell of the workspace;
//   * grand_carry_kernel: one workgroup per argument turns the argument's chunk products into exclusive prefixes in place,
//     writes the closing cell and the argument's 16-byte part of the report;
//   * grand_scan_kernel<NT>: a workgroup makes the factors of its chunk again and scans them from its carry-in: in-lane over the
//     lane's consecutive rows, lanes joined by the wave's scan, waves through LDS; Z leaves through aesw_store.h's flavour;
//   * grand_report_kernel: one workgroup folds the parts into the report (aesw_report_dev.h's workgroup_fold);
//   * the entry points and the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's).
// How a cell lies in memory, moves between lanes and is scanned over a wave is aesw_fr_dev.h's.
// No atomic, no look-back flag, nothing to reset: every word of every output is stored once per call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_grand.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_grand.h"

namespace aesw_grand {
using namespace aesw;

constexpr int THREADS = GRAND_THREADS, ROWS = GRAND_ROWS_PER_LANE, WAVES = THREADS / LANES, BATCH = GRAND_BATCH;
typedef uint32_t index_vec __attribute__((ext_vector_type(ROWS)));  // a lane's rows of an index column: one load
static_assert(sizeof(Fr) == 32 && sizeof(aesw_grand_invert_report) == 3 * sizeof(uint64_t) && sizeof(aesw_grand_report) == 3 * sizeof(uint64_t),
              "a cell is two 16-byte pieces; the kernels address the reports as u64 words");
static_assert(AESW_GRAND_PLANES == GRAND_PLANES, "the header's constant is the rule's");

// Which launches the entry points enqueue: all of them, except in a measurement variant built with -DAESW_GRAND_PASSES=<mask>
// (tests/test_perf_grand.py prices one kernel at a time that way; such a library's outputs are of no use).
#ifndef AESW_GRAND_PASSES
#define AESW_GRAND_PASSES 0x3f
#endif
constexpr unsigned PASSES = AESW_GRAND_PASSES, PASS_INVERT = 1, PASS_INVERT_REPORT = 2, PASS_CHUNK = 4, PASS_CARRY = 8, PASS_SCAN = 16, PASS_REPORT = 32;

// ---- the inverse table ------------------------------------------------------------------------------------------------------

// grid: x = 256 lanes of BATCH rows, y = plane * 3 + table
__global__ void __launch_bounds__(THREADS) grand_invert_kernel(const u32x4 *__restrict__ tables, const u32x4 *__restrict__ beta_cell,
                                                               const u32x4 *__restrict__ gamma_cell, u32x4 *__restrict__ out) {
    const Fr beta = load_cell(beta_cell), gamma = load_cell(gamma_cell);  // one address each for the whole grid
    const bool ok = fr_is_canonical(beta) && fr_is_canonical(gamma);
    const Fr c = blockIdx.y >= THETA_TABLES ? gamma : beta;
    const uint32_t r0 = (blockIdx.x * THREADS + threadIdx.x) * BATCH;
    if (r0 >= MULT_BINS) return;
    const u32x4 *T = tables + (uint64_t)(blockIdx.y % THETA_TABLES) * MULT_BINS * 2;
    u32x4 *O = out + (uint64_t)blockIdx.y * MULT_BINS * 2;
    const auto put = [&](int i, const Fr &v) {
        if (r0 + i < MULT_BINS) store_cell<0>(O + (uint64_t)(r0 + i) * 2, v);
    };
    if (!ok) {
#pragma unroll
        for (int i = 0; i < BATCH; ++i) put(i, FR_ZERO);
        return;
    }
    // a row behind the table counts as a zero sum: skipped by the product, stored nowhere
    grand_batch_invert<BATCH>([&](int i) { return r0 + i < MULT_BINS ? fr_add(load_cell(T + (uint64_t)(r0 + i) * 2), c) : FR_ZERO; }, put);
}

// one workgroup: how many of the 2 x 3 x 66 561 sums are zero
constexpr int REPORT_THREADS = 1024;
__global__ void __launch_bounds__(REPORT_THREADS) grand_invert_report_kernel(const u32x4 *__restrict__ tables, const u32x4 *__restrict__ beta_cell,
                                                                             const u32x4 *__restrict__ gamma_cell, uint64_t *__restrict__ report) {
    __shared__ uint32_t s_sums[1][REPORT_THREADS / LANES];
    __shared__ unsigned long long s_first[REPORT_THREADS / LANES];
    const Fr beta = load_cell(beta_cell), gamma = load_cell(gamma_cell);
    const bool ok = fr_is_canonical(beta) && fr_is_canonical(gamma);
    uint32_t sums[1] = {0};
    unsigned long long first = ~0ull;  // the fold's minimum: not used here
    if (ok) {
        for (uint32_t i = threadIdx.x; i < THETA_TABLES * MULT_BINS; i += REPORT_THREADS) {
            const Fr t = load_cell(tables + (uint64_t)i * 2);
            sums[0] += (fr_is_zero(fr_add(t, beta)) ? 1u : 0u) + (fr_is_zero(fr_add(t, gamma)) ? 1u : 0u);
        }
    }
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) {
        report[0] = (uint64_t)GRAND_PLANES * THETA_TABLES * MULT_BINS;
        report[1] = ok ? 0u : 1u;
        report[2] = sums[0];
    }
}

// ---- the grand product ------------------------------------------------------------------------------------------------------

struct ProductParams {
    const uint32_t *in, *a, *s;    // [n_sets][5][2^k] each
    const u32x4 *tables, *inverses;  // [3][66561] and [2][3][66561] cells
    const u32x4 *beta, *gamma;
    u32x4 *z;        // [n_sets][5][2^k] cells
    u32x4 *carries;  // the workspace: [arguments][stride] cells
    uint32_t k, n_rows, pad_row, last_row, stride;
};

// The factors of the lane's rows i0 ... i0 + ROWS - 1 of argument `arg`; 1 at and behind n_rows.  i0 < 2^k, a multiple of ROWS.
__device__ __forceinline__ void lane_factors(const ProductParams &p, uint32_t arg, uint32_t i0, Fr (&f)[ROWS]) {
#pragma unroll
    for (int q = 0; q < ROWS; ++q) f[q] = FR_ONE;
    if (i0 >= p.n_rows) return;
    const uint32_t j = theta_table_of_tag(arg % THETA_TAGS + 1);  // one per workgroup
    const u32x4 *T = p.tables + (uint64_t)j * MULT_BINS * 2;
    const u32x4 *IA = p.inverses + (uint64_t)j * MULT_BINS * 2, *IS = p.inverses + (uint64_t)(THETA_TABLES + j) * MULT_BINS * 2;
    const Fr beta = load_cell(p.beta), gamma = load_cell(p.gamma);
    const uint64_t at = ((uint64_t)arg << p.k) + i0;
    const index_vec vin = *reinterpret_cast<const index_vec *>(p.in + at), va = *reinterpret_cast<const index_vec *>(p.a + at),
                    vs = *reinterpret_cast<const index_vec *>(p.s + at);
    fr_unrolled<ROWS>([&](auto at) {
        constexpr int q = decltype(at)::value;
        if (i0 + q < p.n_rows)
            f[q] = grand_row(load_cell(T + grand_row_of_index(vin[q]) * 2), load_cell(T + theta_table_index(i0 + q, p.pad_row) * 2),
                             load_cell(IA + grand_row_of_index(va[q]) * 2), load_cell(IS + grand_row_of_index(vs[q]) * 2), beta, gamma);
    });
}

// grid: x = the chunk, y = the argument
__global__ void __launch_bounds__(THREADS) grand_chunk_kernel(const ProductParams p) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t arg = blockIdx.y, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    Fr f[ROWS];
    lane_factors(p, arg, blockIdx.x * GRAND_CHUNK + threadIdx.x * ROWS, f);
    Fr t = f[0];
    fr_unrolled<ROWS - 1>([&](auto at) { t = fr_mul(t, f[decltype(at)::value + 1]); });
#pragma unroll 1
    for (int o = LANES / 2; o; o >>= 1) t = fr_mul(t, shfl_xor_cell(t, o));  // the field is commutative: a butterfly will do
    if (lane == 0) s_wave[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int w = 1; w < WAVES; ++w) t = fr_mul(t, s_wave[w]);
        store_cell<0>(cell_at(p.carries, (uint64_t)arg * p.stride + blockIdx.x), t);
    }
}

// grid: x = the argument.  Its chunk products -> exclusive prefixes, in place, 256 chunks a turn.
__global__ void __launch_bounds__(THREADS) grand_carry_kernel(u32x4 *__restrict__ carries, uint32_t stride, uint32_t chunks, u32x4 *__restrict__ closing,
                                                              u32x4 *__restrict__ parts) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t arg = blockIdx.x, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    u32x4 *cells = cell_at(carries, (uint64_t)arg * stride);
    Fr running = FR_ONE;  // the product of every chunk below this turn's, in every thread
    for (uint32_t first = 0; first < chunks; first += THREADS) {
        const uint32_t i = first + threadIdx.x;
        const Fr incl = wave_scan_up(i < chunks ? load_cell(cell_at(cells, i)) : FR_ONE, lane);
        Fr excl = shfl_up_cell(incl, 1);
        if (lane == 0) excl = FR_ONE;
        if (lane == LANES - 1) s_wave[wave] = incl;
        __syncthreads();
        Fr base = running;
#pragma unroll 1
        for (uint32_t w = 0; w < WAVES; ++w) {
            if (w == wave) base = running;  // what lies below this wave
            running = fr_mul(running, s_wave[w]);
        }
        if (i < chunks) store_cell<0>(cell_at(cells, i), fr_mul(base, excl));
        __syncthreads();  // s_wave is written again next turn
    }
    if (threadIdx.x == 0) {
        store_cell<0>(cell_at(closing, arg), running);
        const bool open = !fr_eq(running, FR_ONE);
        const uint64_t key = open ? grand_argument_key(arg) : ~0ull;
        parts[arg] = u32x4{open ? 1u : 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32)};
    }
}

// grid: x = the chunk, y = the argument.  A lane writes 32 * ROWS contiguous bytes.
template <int NT>
__global__ void __launch_bounds__(THREADS) grand_scan_kernel(const ProductParams p) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t arg = blockIdx.y, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const uint32_t i0 = blockIdx.x * GRAND_CHUNK + threadIdx.x * ROWS;
    Fr f[ROWS];
    lane_factors(p, arg, i0, f);
    fr_unrolled<ROWS - 1>([&](auto at) { f[decltype(at)::value + 1] = fr_mul(f[decltype(at)::value], f[decltype(at)::value + 1]); });  // inclusive, in the lane
    const Fr incl = wave_scan_up(f[ROWS - 1], lane);
    Fr excl = shfl_up_cell(incl, 1);
    if (lane == 0) excl = FR_ONE;
    if (lane == LANES - 1) s_wave[wave] = incl;
    __syncthreads();
    Fr base = load_cell(cell_at(p.carries, (uint64_t)arg * p.stride + blockIdx.x));  // the carry-in: Z at the chunk's first row
#pragma unroll 1
    for (uint32_t w = 0; w < wave; ++w) base = fr_mul(base, s_wave[w]);
    base = fr_mul(base, excl);  // Z[i0]
    u32x4 *z = cell_at(p.z, ((uint64_t)arg << p.k) + i0);
    if (i0 <= p.last_row) store_cell<NT>(z, base);
    fr_unrolled<ROWS - 1>([&](auto at) {
        constexpr int q = decltype(at)::value + 1;
        if (i0 + q <= p.last_row) store_cell<NT>(cell_at(z, q), fr_mul(base, f[q - 1]));
    });
}

// one workgroup: the arguments' parts into the report
__global__ void __launch_bounds__(REPORT_THREADS) grand_report_kernel(const u32x4 *__restrict__ parts, uint32_t n_parts, uint64_t *__restrict__ report) {
    __shared__ unsigned long long s_sums[1][REPORT_THREADS / LANES], s_first[REPORT_THREADS / LANES];
    unsigned long long sums[1] = {0}, first = ~0ull;  // open
    for (uint32_t i = threadIdx.x; i < n_parts; i += REPORT_THREADS) {
        const u32x4 v = parts[i];
        const unsigned long long f = (unsigned long long)v[3] << 32 | v[2];
        sums[0] += v[0];
        first = f < first ? f : first;
    }
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) { report[0] = n_parts; report[1] = sums[0]; report[2] = first; }
}

}  // namespace aesw_grand

extern "C" {

int aesw_grand_invert_table_device(aesw_ctx *ctx, const uint8_t *d_table_fr, const uint8_t *d_beta, const uint8_t *d_gamma, uint8_t *d_inv_fr,
                                   aesw_grand_invert_report *d_report, void *stream) {
    using namespace aesw_grand;
    const char *const call = "aesw_grand_invert_table_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!d_table_fr || !aligned_to(d_table_fr, 16)) return refuse(ctx, call, "d_table_fr must be there and 16-byte aligned");
    if (const char *why = bad_challenges(d_beta, d_gamma)) return refuse(ctx, call, why);
    if (!d_inv_fr || !aligned_to(d_inv_fr, 16)) return refuse(ctx, call, "d_inv_fr must be there and 16-byte aligned");
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u32x4 *tables = reinterpret_cast<const u32x4 *>(d_table_fr), *beta = reinterpret_cast<const u32x4 *>(d_beta), *gamma = reinterpret_cast<const u32x4 *>(d_gamma);
    const uint32_t lanes = (MULT_BINS + BATCH - 1) / BATCH;
    if constexpr (PASSES & PASS_INVERT)
        hipLaunchKernelGGL(grand_invert_kernel, dim3((lanes + THREADS - 1) / THREADS, GRAND_PLANES * THETA_TABLES), dim3(THREADS), 0, s, tables, beta, gamma,
                           reinterpret_cast<u32x4 *>(d_inv_fr));
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_INVERT_REPORT)
        hipLaunchKernelGGL(grand_invert_report_kernel, dim3(1), dim3(REPORT_THREADS), 0, s, tables, beta, gamma, reinterpret_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

size_t aesw_grand_workspace_bytes(uint32_t k, uint32_t n_sets) { return (size_t)aesw::grand_workspace_bytes(k, n_sets); }

int aesw_grand_product_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row, const uint32_t *d_in, const uint32_t *d_a,
                              const uint32_t *d_s, const uint8_t *d_table_fr, const uint8_t *d_inv_fr, const uint8_t *d_beta, const uint8_t *d_gamma,
                              uint8_t *d_z_fr, uint8_t *d_closing_fr, void *d_workspace, aesw_grand_report *d_report, void *stream) {
    using namespace aesw_grand;
    const char *const call = "aesw_grand_product_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!grand_k_ok(k)) return refuse(ctx, call, "k must be 17 ... 30 (2^k rows hold the table)");
    if (const char *why = bad_sets(n_sets)) return refuse(ctx, call, why);
    if (n_rows < MULT_BINS || n_rows > (1u << k)) return refuse(ctx, call, "n_rows must be 66561 ... 2^k");
    if (pad_row >= MULT_BINS) return refuse(ctx, call, "pad_row must be a table row, 0 ... 66560");
    if (!d_in || !d_a || !d_s || !aligned_to(d_in, 16) || !aligned_to(d_a, 16) || !aligned_to(d_s, 16))
        return refuse(ctx, call, "d_in, d_a and d_s must be there and 16-byte aligned");
    if (!d_table_fr || !d_inv_fr || !aligned_to(d_table_fr, 16) || !aligned_to(d_inv_fr, 16))
        return refuse(ctx, call, "d_table_fr and d_inv_fr must be there and 16-byte aligned");
    if (const char *why = bad_challenges(d_beta, d_gamma)) return refuse(ctx, call, why);
    if (const char *why = bad_product_outputs(d_z_fr, d_closing_fr)) return refuse(ctx, call, why);
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t n_args = n_sets * THETA_TAGS, chunks = grand_chunks(k, n_rows);  // <= 5 120 and <= 2^20: both fit a grid
    ProductParams p{};
    p.in = d_in; p.a = d_a; p.s = d_s;
    p.tables = reinterpret_cast<const u32x4 *>(d_table_fr);
    p.inverses = reinterpret_cast<const u32x4 *>(d_inv_fr);
    p.beta = reinterpret_cast<const u32x4 *>(d_beta);
    p.gamma = reinterpret_cast<const u32x4 *>(d_gamma);
    p.z = reinterpret_cast<u32x4 *>(d_z_fr);
    p.carries = static_cast<u32x4 *>(d_workspace);
    p.k = k; p.n_rows = n_rows; p.pad_row = pad_row;
    p.last_row = grand_last_row(k, n_rows);
    p.stride = grand_chunk_stride(k);
    u32x4 *parts = p.carries + grand_workspace_cells(k, n_sets) * 2;
    const dim3 grid(chunks, n_args);
    if constexpr (PASSES & PASS_CHUNK) hipLaunchKernelGGL(grand_chunk_kernel, grid, dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CARRY)
        hipLaunchKernelGGL(grand_carry_kernel, dim3(n_args), dim3(THREADS), 0, s, p.carries, p.stride, chunks, reinterpret_cast<u32x4 *>(d_closing_fr), parts);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_SCAN) with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(grand_scan_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, p); });
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_REPORT) hipLaunchKernelGGL(grand_report_kernel, dim3(1), dim3(REPORT_THREADS), 0, s, parts, n_args, reinterpret_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
