// msm/aesw_msm.hip -- libaesw_msm.so (include/aesw_msm.h): columns of scalars committed against a basis of points of bn256's G1,
// on the device.  The fields are aesw_fq.h's and aesw_fr.h's and the rules -- the point forms, the one addition
// law, the windows, the slices and the chunks, the workspace -- are aesw_msm.h's; nothing of them is restated here.  What is here:
//   * msm_basis_kernel: a thread takes one point's plain coordinates to Montgomery form and checks them in the same pass;
//   * msm_digits_kernel: a thread takes one cell to its plain value and writes its 32 bytes to the 32 planes of the workspace;
//   * msm_bucket_kernel: a workgroup owns one slice of one window of one column, thread b its bucket b in registers; per chunk a
//     counting sort of the row indices by digit in LDS, then every thread walks its own list and adds the listed basis points;
//   * msm_reduce_kernel: a workgroup per window and column sums the slices bucket by bucket and forms sum_b b * B_b as the sum
//     of the suffix sums: one suffix scan and one reduction of point additions over 256 threads;
//   * msm_combine_kernel: a lane per column, Horner over the windows, one inversion, 64 bytes stored;
//   * the entry points and the checks that are theirs alone.
// No global atomic but the report's: every word of the workspace and of the output is stored once per call, the passes are
// ordered by the stream.  The order in which a bucket meets its points is not fixed (the LDS cursor), the sum is: the group is
// commutative and the law exact, so the affine result is the same bytes on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_msm.h"
#include "../aesw_check_dev.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_msm.h"

namespace aesw_msm {
using namespace aesw;

constexpr int THREADS = MSM_THREADS, WAVES = MSM_WAVES;
static_assert(MSM_LANES == LANES && sizeof(Fq) == 32, "the rules count the lanes of a wave as the device does; a coordinate is two 16-byte pieces");
static_assert(AESW_MSM_FR == MSM_SCALARS_FR && AESW_MSM_BYTES == MSM_SCALARS_BYTES, "the header's scalar kinds are the rules'");

// Which launches aesw_msm_commit_device enqueues: all of them, except in a measurement variant built with
// -DAESW_MSM_PASSES=<mask> (tools/msm_bench.py prices one kernel at a time that way; such a library's outputs are of no use).
#ifndef AESW_MSM_PASSES
#define AESW_MSM_PASSES 0xf
#endif
constexpr unsigned PASSES = AESW_MSM_PASSES, PASS_DIGITS = 1, PASS_BUCKET = 2, PASS_REDUCE = 4, PASS_COMBINE = 8;

// ---- a coordinate, a point and memory ------------------------------------------------------------------------------------------

__device__ __forceinline__ Fq load_fq(const u32x4 *p) {
    const u32x4 lo = p[0], hi = p[1];
    return Fq{{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
}
__device__ __forceinline__ void store_fq(u32x4 *p, const Fq &v) {
    p[0] = u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
    p[1] = u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
}
__device__ __forceinline__ G1Affine load_affine(const u32x4 *base, uint64_t i) { return G1Affine{load_fq(base + i * 4), load_fq(base + i * 4 + 2)}; }
__device__ __forceinline__ void store_affine(u32x4 *base, uint64_t i, const G1Affine &p) {
    store_fq(base + i * 4, p.x);
    store_fq(base + i * 4 + 2, p.y);
}
__device__ __forceinline__ G1 load_point(const u32x4 *base, uint64_t i) { return G1{load_fq(base + i * 6), load_fq(base + i * 6 + 2), load_fq(base + i * 6 + 4)}; }
__device__ __forceinline__ void store_point(u32x4 *base, uint64_t i, const G1 &p) {
    store_fq(base + i * 6, p.x);
    store_fq(base + i * 6 + 2, p.y);
    store_fq(base + i * 6 + 4, p.z);
}

__device__ __forceinline__ Fq shfl_down_fq(const Fq &v, int o) {
    Fq r = FQ_ZERO;
#pragma unroll
    for (int i = 0; i < FQ_LIMBS; ++i) r.l[i] = __shfl_down(v.l[i], o, LANES);
    return r;
}
__device__ __forceinline__ Fq shfl_xor_fq(const Fq &v, int o) {
    Fq r = FQ_ZERO;
#pragma unroll
    for (int i = 0; i < FQ_LIMBS; ++i) r.l[i] = __shfl_xor(v.l[i], o, LANES);
    return r;
}
__device__ __forceinline__ G1 shfl_down_point(const G1 &p, int o) { return G1{shfl_down_fq(p.x, o), shfl_down_fq(p.y, o), shfl_down_fq(p.z, o)}; }
__device__ __forceinline__ G1 shfl_xor_point(const G1 &p, int o) { return G1{shfl_xor_fq(p.x, o), shfl_xor_fq(p.y, o), shfl_xor_fq(p.z, o)}; }

// ---- the basis ------------------------------------------------------------------------------------------------------------------

// words 0 and 1 of the report: the bad points, the first of them (~0: none)
__global__ void __launch_bounds__(LANES) msm_report_reset_kernel(uint64_t *report) { report_reset(report, 2, 1u << 1, threadIdx.x); }

// grid: x = 256 points.  A point that fails is stored as it came out, and counted.
__global__ void __launch_bounds__(THREADS) msm_basis_kernel(const u32x4 *__restrict__ canonical, u32x4 *__restrict__ basis, uint64_t *__restrict__ report) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;  // below 2^k: a basis is whole workgroups
    const G1Affine raw = load_affine(canonical, i);
    const G1Affine p{fq_mul(raw.x, FQ_R2), fq_mul(raw.y, FQ_R2)};
    const bool good = fq_is_canonical(raw.x) && fq_is_canonical(raw.y) && msm_on_curve(p);
    store_affine(basis, i, p);
    report_add(report, good ? 0u : 1u);
    report_min(report + 1, good ? ~0ull : (uint64_t)i);
}

// ---- the digits -----------------------------------------------------------------------------------------------------------------

// grid: x = 256 rows, y = the column.  The cell is read once; byte w of its plain value goes to plane w.
__global__ void __launch_bounds__(THREADS) msm_digits_kernel(const u32x4 *__restrict__ cells, uint8_t *__restrict__ planes, uint32_t k) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const Fr s = msm_canonical_scalar(load_cell(cell_at(cells, ((uint64_t)blockIdx.y << k) + i)));
    uint8_t *at = planes + msm_plane_at(k, blockIdx.y, 0) + i;
#pragma unroll
    for (int w = 0; w < (int)MSM_FR_WINDOWS; ++w) at[(uint64_t)w << k] = (uint8_t)(s.l[w / 4] >> (8 * (w % 4)));
}

// ---- the buckets ----------------------------------------------------------------------------------------------------------------

struct BucketParams {
    const uint8_t *digits;  // the planes of the workspace, or the byte columns themselves
    const u32x4 *basis;     // [2^k] affine points
    u32x4 *buckets;         // the workspace's buckets
    uint32_t k, windows, plane_windows;  // plane_windows: the planes a column has in `digits` (32, or 1 for byte columns)
};

// grid: x = the slice, y = the window, z = the column.
__global__ void __launch_bounds__(THREADS) msm_bucket_kernel(const BucketParams p) {
    __shared__ uint32_t s_count[MSM_BUCKETS];   // the histogram of the chunk, then every bucket's cursor
    __shared__ uint32_t s_wave[WAVES];          // the rows of every wave's buckets
    __shared__ uint16_t s_rows[MSM_CHUNK];      // the rows of the chunk, sorted by digit
    const uint32_t b = threadIdx.x, lane = b % LANES, wave = b / LANES, slices = gridDim.x;
    const uint32_t begin = msm_slice_begin(p.k, slices, blockIdx.x), end = msm_slice_begin(p.k, slices, blockIdx.x + 1);
    const uint8_t *plane = p.digits + ((((uint64_t)blockIdx.z * p.plane_windows) + blockIdx.y) << p.k);
    G1 acc = msm_identity();
#pragma unroll 1
    for (uint32_t at = begin; at < end; at += MSM_CHUNK) {
        s_count[b] = 0;
        __syncthreads();
        // word j * 256 + b of the chunk: four rows; a slice begins and ends at a multiple of 16 rows, so a word is whole or absent
        uint32_t words[MSM_WORDS_PER_THREAD];
#pragma unroll
        for (uint32_t j = 0; j < MSM_WORDS_PER_THREAD; ++j) {
            const uint32_t row = at + (j * THREADS + b) * 4;
            words[j] = row < end ? *reinterpret_cast<const uint32_t *>(plane + row) : 0u;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t d = words[j] >> (8 * q) & 0xffu;
                if (d) atomicAdd(&s_count[d], 1u);
            }
        }
        __syncthreads();
        // the exclusive prefix of the 256 counts: the wave by shuffles, the four waves through LDS
        const uint32_t count = s_count[b];
        uint32_t incl = count;
#pragma unroll
        for (int o = 1; o < LANES; o <<= 1) {
            const uint32_t other = __shfl_up(incl, o, LANES);
            if (lane >= (uint32_t)o) incl += other;
        }
        if (lane == LANES - 1) s_wave[wave] = incl;
        __syncthreads();
        uint32_t first = incl - count;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) first += w < wave ? s_wave[w] : 0u;
        s_count[b] = first;  // every thread read its own count above, and no other's
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < MSM_WORDS_PER_THREAD; ++j) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t d = words[j] >> (8 * q) & 0xffu;
                if (d) s_rows[atomicAdd(&s_count[d], 1u)] = (uint16_t)((j * THREADS + b) * 4 + q);  // below first + count of bucket d: at most MSM_CHUNK in all
            }
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t i = first; i < first + count; ++i) acc = msm_add_mixed(acc, load_affine(p.basis, at + s_rows[i]));
        __syncthreads();  // s_rows and s_count are written again next chunk
    }
    store_point(p.buckets, msm_bucket_at(p.windows, slices, blockIdx.z, blockIdx.y, blockIdx.x, b), acc);
}

// ---- a window's sum ---------------------------------------------------------------------------------------------------------------

// grid: x = the window, y = the column.
__global__ void __launch_bounds__(THREADS) msm_reduce_kernel(const u32x4 *__restrict__ buckets, u32x4 *__restrict__ sums, uint32_t slices) {
    __shared__ u32x4 s_wave[WAVES * 6];
    const uint32_t b = threadIdx.x, lane = b % LANES, wave = b / LANES, windows = gridDim.x;
    G1 v = msm_identity();
#pragma unroll 1
    for (uint32_t s = 0; s < slices; ++s) v = msm_add(v, load_point(buckets, msm_bucket_at(windows, slices, blockIdx.y, blockIdx.x, s, b)));
    // the inclusive suffix scan: thread b ends with S_b = B_b + ... + B_255.  Every lane shuffles and adds; the lanes that have a partner keep the sum.
#pragma unroll 1
    for (int o = 1; o < LANES; o <<= 1) {
        const G1 sum = msm_add(v, shfl_down_point(v, o));
        v = msm_select(lane + (uint32_t)o < (uint32_t)LANES, sum, v);
    }
    if (lane == 0) store_point(s_wave, wave, v);
    __syncthreads();
#pragma unroll 1
    for (uint32_t w = WAVES - 1; w > 0; --w) {  // the waves above this one
        const G1 sum = msm_add(v, load_point(s_wave, w));
        v = msm_select(w > wave, sum, v);
    }
    v = msm_select(b == 0, msm_identity(), v);  // S_0 is no term: the sum runs over j = 1 ... 255
    // the reduction of the 256 suffix sums
#pragma unroll 1
    for (int o = LANES / 2; o; o >>= 1) v = msm_add(v, shfl_xor_point(v, o));
    __syncthreads();  // every thread has read s_wave
    if (lane == 0) store_point(s_wave, wave, v);
    __syncthreads();
    if (b == 0) {
#pragma unroll 1
        for (uint32_t w = 1; w < (uint32_t)WAVES; ++w) v = msm_add(v, load_point(s_wave, w));
        store_point(sums, msm_sum_at(windows, blockIdx.y, blockIdx.x), v);
    }
}

// ---- the commitment ---------------------------------------------------------------------------------------------------------------

// grid: x = 64 columns.  Horner over the windows from the top.
__global__ void __launch_bounds__(LANES) msm_combine_kernel(const u32x4 *__restrict__ sums, u32x4 *__restrict__ out, uint32_t windows, uint32_t n_cols) {
    const uint32_t c = blockIdx.x * LANES + threadIdx.x;
    if (c >= n_cols) return;
    G1 acc = load_point(sums, msm_sum_at(windows, c, windows - 1));
#pragma unroll 1
    for (uint32_t w = windows - 1; w-- > 0;) {
#pragma unroll 1
        for (uint32_t d = 0; d < MSM_WINDOW_BITS; ++d) acc = msm_double(acc);
        acc = msm_add(acc, load_point(sums, msm_sum_at(windows, c, w)));
    }
    store_affine(out, c, msm_to_affine(acc));
}

// ---- the checks -----------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }

}  // namespace aesw_msm

extern "C" {

size_t aesw_msm_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices) { return (size_t)aesw::msm_workspace_bytes(k, n_cols, scalars, slices); }

uint32_t aesw_msm_chunk_rows(void) { return aesw::MSM_CHUNK; }

uint32_t aesw_msm_slices(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices) {
    using namespace aesw;
    return msm_k_ok(k) && msm_cols_ok(n_cols) && msm_scalars_ok(scalars) && msm_slices_ok(k, slices) ? msm_slices(k, n_cols, scalars, slices) : 0u;
}

int aesw_msm_basis_device(aesw_ctx *ctx, uint32_t k, const uint8_t *d_canonical, uint8_t *d_basis, aesw_msm_report *d_report, void *stream) {
    using namespace aesw_msm;
    const char *const call = "aesw_msm_basis_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!msm_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (bad_pointer(d_canonical)) return refuse(ctx, call, "d_canonical must be there and 16-byte aligned");
    if (bad_pointer(d_basis)) return refuse(ctx, call, "d_basis must be there and 16-byte aligned");
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    const uint64_t bytes = sizeof(G1Affine) << k;
    if (d_basis != d_canonical && overlap(d_basis, bytes, d_canonical, bytes)) return refuse(ctx, call, "d_basis must be d_canonical itself or must not overlap it");
    if (overlap(d_report, sizeof(aesw_msm_report), d_basis, bytes) || overlap(d_report, sizeof(aesw_msm_report), d_canonical, bytes))
        return refuse(ctx, call, "d_report must not overlap d_canonical or d_basis");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t *report = reinterpret_cast<uint64_t *>(d_report);
    hipLaunchKernelGGL(msm_report_reset_kernel, dim3(1), dim3(LANES), 0, s, report);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(msm_basis_kernel, dim3((1u << k) / THREADS), dim3(THREADS), 0, s, reinterpret_cast<const u32x4 *>(d_canonical), reinterpret_cast<u32x4 *>(d_basis),
                       report);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_msm_commit_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices, const uint8_t *d_scalars, const uint8_t *d_basis,
                           uint8_t *d_out, void *d_workspace, void *stream) {
    using namespace aesw_msm;
    const char *const call = "aesw_msm_commit_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!msm_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (!msm_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 65535");
    if (!msm_scalars_ok(scalars)) return refuse(ctx, call, "scalars must be AESW_MSM_FR or AESW_MSM_BYTES");
    if (!msm_slices_ok(k, slices)) return refuse(ctx, call, "slices must be 0 (the rule's) ... 2^k / 16, at most 65535");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_basis)) return refuse(ctx, call, "d_basis must be there and 16-byte aligned");
    if (bad_pointer(d_out)) return refuse(ctx, call, "d_out must be there and 16-byte aligned");
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    const uint32_t windows = msm_windows(scalars), sl = msm_slices(k, n_cols, scalars, slices);
    const uint64_t scalars_bytes = ((uint64_t)n_cols << k) * (scalars == MSM_SCALARS_FR ? sizeof(Fr) : 1u), basis_bytes = sizeof(G1Affine) << k,
                   out_bytes = (uint64_t)n_cols * sizeof(G1Affine), ws_bytes = msm_workspace_bytes(k, n_cols, scalars, slices);
    if (overlap(d_out, out_bytes, d_scalars, scalars_bytes) || overlap(d_out, out_bytes, d_basis, basis_bytes)) return refuse(ctx, call, "d_out must not overlap d_scalars or d_basis");
    if (overlap(d_workspace, ws_bytes, d_out, out_bytes) || overlap(d_workspace, ws_bytes, d_scalars, scalars_bytes) || overlap(d_workspace, ws_bytes, d_basis, basis_bytes))
        return refuse(ctx, call, "d_workspace must not overlap d_out, d_scalars or d_basis");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    u32x4 *buckets = reinterpret_cast<u32x4 *>(ws + msm_planes_bytes(k, n_cols, scalars));  // the planes are a multiple of 1 024 bytes
    u32x4 *sums = buckets + msm_bucket_at(windows, sl, n_cols, 0, 0, 0) * (sizeof(G1) / sizeof(u32x4));
    BucketParams p{};
    p.digits = scalars == MSM_SCALARS_FR ? ws : d_scalars;
    p.basis = reinterpret_cast<const u32x4 *>(d_basis);
    p.buckets = buckets;
    p.k = k; p.windows = windows; p.plane_windows = windows;
    if constexpr (PASSES & PASS_DIGITS)
        if (scalars == MSM_SCALARS_FR) hipLaunchKernelGGL(msm_digits_kernel, dim3((1u << k) / THREADS, n_cols), dim3(THREADS), 0, s, reinterpret_cast<const u32x4 *>(d_scalars), ws, k);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_BUCKET) hipLaunchKernelGGL(msm_bucket_kernel, dim3(sl, windows, n_cols), dim3(THREADS), 0, s, p);  // <= 65535 slices and columns
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_REDUCE) hipLaunchKernelGGL(msm_reduce_kernel, dim3(windows, n_cols), dim3(THREADS), 0, s, buckets, sums, sl);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_COMBINE)
        hipLaunchKernelGGL(msm_combine_kernel, dim3((n_cols + LANES - 1) / LANES), dim3(LANES), 0, s, sums, reinterpret_cast<u32x4 *>(d_out), windows, n_cols);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
