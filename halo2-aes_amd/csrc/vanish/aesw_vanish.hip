// vanish/aesw_vanish.hip -- libaesw_vanish.so (include/aesw_vanish.h): the quotient h(X) folded on the device one constraint
// segment per call.  The field is aesw_fr.h's; the bounds, the rotations, the tables and x_j are aesw_quot.h's;
// the segments, their order and the scalars block are aesw_vanish.h's; nothing of the three is restated here.  What is here:
//   * vanish_tables_kernel: a thread writes one cell of the tables;
//   * vanish_scalars_kernel, one workgroup: a thread writes a cell of the scalars block from the four challenges;
//   * vanish_head_kernel<NT>, vanish_perm_kernel<NT>, vanish_lookup_kernel<NT>: a lane per extended row runs the header's segment over
//     its own columns and stores its cell of acc; a rotated cell is read again through the cache (the -DAESW_VANISH_LDS=1 variant
//     of the lookup kernel, which stages it through LDS, measured 1.45 times slower: 4.33);
//   * vanish_divide_kernel<NT>: a lane multiplies its cell by the vanishing table's;
//   * the entry points and their checks.
// No atomic, no LDS in the shipped build, no workspace: every output cell is stored once by the lane that owns it, which is also the only one that
// reads that cell of acc_in -- so acc_in may be acc_out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_vanish.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_quot.h"
#include "../aesw_vanish.h"

namespace aesw_vanish {
using namespace aesw;

constexpr uint32_t THREADS = QUOT_THREADS;
static_assert(sizeof(Fr) == 32, "a cell is two 16-byte pieces");
static_assert((1u << (QUOT_MIN_K + QUOT_MIN_LOG_M)) % THREADS == 0, "the smallest extended column is whole workgroups");

// cell `row` of column `column` of a group [columns][2^ext_k] cells
__device__ __forceinline__ Fr group_cell(const u32x4 *group, uint32_t column, uint32_t ext_k, uint32_t row) {
    return load_cell(cell_at(group, ((uint64_t)column << ext_k) + row));
}

// ---- the two small kernels ----------------------------------------------------------------------------------------------------------

// grid: x = ceil(cells / THREADS)
__global__ void __launch_bounds__(THREADS) vanish_tables_kernel(u32x4 *tables, uint32_t k, uint32_t ext_k, uint32_t zeta_sel) {
    const uint32_t at = blockIdx.x * THREADS + threadIdx.x;
    if (at < quot_tables(k, ext_k).cells) store_cell<0>(cell_at(tables, at), quot_table_cell(k, ext_k, zeta_sel, at));
}

// one workgroup
__global__ void __launch_bounds__(THREADS) vanish_scalars_kernel(const u32x4 *__restrict__ theta, const u32x4 *__restrict__ beta, const u32x4 *__restrict__ gamma,
                                                                  const u32x4 *__restrict__ y, u32x4 *__restrict__ scalars, uint32_t n_sets, uint32_t chunk_len) {
    const Fr t = load_cell(theta), b = load_cell(beta), g = load_cell(gamma), v = load_cell(y);
#pragma unroll 1
    for (uint32_t at = threadIdx.x; at < vanish_scalars_cells(n_sets, chunk_len); at += THREADS)
        store_cell<0>(cell_at(scalars, at), vanish_scalar_cell(at, n_sets, chunk_len, t, b, g, v));
}

// ---- the segments: grid x = 2^ext_k / THREADS, a lane per row -------------------------------------------------------------------------

struct HeadParams {
    const u32x4 *words, *rcon, *zperm, *l, *scalars;
    u32x4 *out;
    QuotShape q;
};
template <int NT>
__global__ void __launch_bounds__(THREADS) vanish_head_kernel(const HeadParams p) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x, ext_k = p.q.ext_k;
    const Fr acc = vanish_head(
        p.q, j,
        [&](uint32_t group, uint32_t column, uint32_t row) {
            return group == QUOT_ADVICE ? group_cell(p.words, 0, ext_k, row)  // the one advice column HEAD reads
                 : group == QUOT_RCON ? group_cell(p.rcon, column, ext_k, row)
                 : group == QUOT_ZPERM ? group_cell(p.zperm, column, ext_k, row) : group_cell(p.l, column, ext_k, row);
        },
        [&](uint32_t at) { return load_cell(cell_at(p.scalars, at)); });
    store_cell<NT>(cell_at(p.out, j), acc);
}

struct PermParams {
    const u32x4 *values, *sigma, *z, *l, *tables, *scalars, *acc;
    u32x4 *out;
    QuotShape q;
    uint32_t set;
};
template <int NT>
__global__ void __launch_bounds__(THREADS) vanish_perm_kernel(const PermParams p) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x, ext_k = p.q.ext_k, first = sigma_set_first(p.set, p.q.chunk_len);
    const Fr x = quot_point(p.q.k, ext_k, j, [&](uint32_t at) { return load_cell(cell_at(p.tables, at)); });
    const Fr acc = vanish_perm(
        p.q, p.set, j, load_cell(cell_at(p.acc, j)), x,
        [&](uint32_t group, uint32_t column, uint32_t row) {
            return group == VANISH_VALUES ? group_cell(p.values, column - first, ext_k, row)
                 : group == QUOT_SIGMA ? group_cell(p.sigma, column - first, ext_k, row)
                 : group == QUOT_ZPERM ? group_cell(p.z, 0, ext_k, row) : group_cell(p.l, column, ext_k, row);
        },
        [&](uint32_t at) { return load_cell(cell_at(p.scalars, at)); });
    store_cell<NT>(cell_at(p.out, j), acc);
}

struct LookupParams {
    const u32x4 *advice, *selectors, *table, *a, *s, *z, *l, *scalars, *acc;
    u32x4 *out;
    QuotShape q;
    uint32_t set;
};
#ifndef AESW_VANISH_LDS
#define AESW_VANISH_LDS 0  // 1: a measurement variant (tools/vanish_bench.py) -- Z[next] and A'[prev] of the lookup kernel staged through LDS
#endif
template <int NT>
__global__ void __launch_bounds__(THREADS) vanish_lookup_kernel(const LookupParams p) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x, ext_k = p.q.ext_k, words = 3u * p.set, args = THETA_TAGS * p.set;
#if AESW_VANISH_LDS
    // The workgroup's 256 rows hold Z[next] for all but its last m lanes and A'[prev] for all but its first m: the lane that reads
    // its own cell of Z or A' leaves it in LDS, the lane m rows below or above takes it from there after a barrier, and the m
    // lanes at the edge read global memory as before.  Every lane runs every tag, so the barriers are met by all.
    __shared__ u32x4 s_z[THREADS][2], s_a[THREADS][2];
    const uint32_t tid = threadIdx.x, m = quot_m(p.q.k, ext_k);
    const auto staged = [&](const u32x4 *group, uint32_t column, uint32_t row, u32x4 (*slot)[2], bool inside, uint32_t from) {
        if (row == j) {  // the lane's own cell: read once, left for the neighbour
            const Fr own = group_cell(group, column, ext_k, row);
            slot[tid][0] = u32x4{own.l[0], own.l[1], own.l[2], own.l[3]};
            slot[tid][1] = u32x4{own.l[4], own.l[5], own.l[6], own.l[7]};
            return own;
        }
        __syncthreads();
        Fr other = FR_ZERO;
        if (inside) {
            const u32x4 lo = slot[from][0], hi = slot[from][1];
            other = Fr{{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
        } else {
            other = group_cell(group, column, ext_k, row);
        }
        __syncthreads();  // the slots are written again at the next tag
        return other;
    };
#endif
    const Fr acc = vanish_lookup(
        p.q, p.set, j, load_cell(cell_at(p.acc, j)),
        [&](uint32_t group, uint32_t column, uint32_t row) {
#if AESW_VANISH_LDS
            if (group == QUOT_ZLOOKUP) return staged(p.z, column - args, row, s_z, tid + m < THREADS, (tid + m) % THREADS);
            if (group == QUOT_A) return staged(p.a, column - args, row, s_a, tid >= m, (tid - m) % THREADS);
#endif
            return group == QUOT_ADVICE ? group_cell(p.advice, column - words, ext_k, row)
                 : group == QUOT_SELECTOR ? group_cell(p.selectors, column - args, ext_k, row)
                 : group == QUOT_TABLE ? group_cell(p.table, column, ext_k, row)
                 : group == QUOT_A ? group_cell(p.a, column - args, ext_k, row)
                 : group == QUOT_S ? group_cell(p.s, column - args, ext_k, row)
                 : group == QUOT_ZLOOKUP ? group_cell(p.z, column - args, ext_k, row) : group_cell(p.l, column, ext_k, row);
        },
        [&](uint32_t at) { return load_cell(cell_at(p.scalars, at)); });
    store_cell<NT>(cell_at(p.out, j), acc);
}

template <int NT>
__global__ void __launch_bounds__(THREADS) vanish_divide_kernel(const u32x4 *tables, const u32x4 *acc, u32x4 *out, uint32_t k, uint32_t ext_k) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x;
    store_cell<NT>(cell_at(out, j), vanish_divide(k, ext_k, j, load_cell(cell_at(acc, j)), [&](uint32_t at) { return load_cell(cell_at(tables, at)); }));
}

// ---- the checks -------------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }
inline uint64_t group_bytes(uint32_t ext_k, uint32_t columns) { return ((uint64_t)columns << ext_k) * sizeof(Fr); }
inline const u32x4 *cells(const uint8_t *p) { return reinterpret_cast<const u32x4 *>(p); }
inline u32x4 *cells(uint8_t *p) { return reinterpret_cast<u32x4 *>(p); }
constexpr const char *SHAPE = "k must be 10 ... 28 and ext_k k + 2 ... 28, n_sets 1 ... 1024, chunk_len 1 ... 8 with chunk_len + 2 <= 2^(ext_k - k) + 1, n_rows 1 ... 2^k - 1";

struct Input {
    const void *p;
    uint64_t bytes;
};
// the first input acc_out overlaps, or -1; acc_in itself may be acc_out
template <size_t N>
inline int first_overlap(const void *out, uint64_t out_bytes, const Input (&in)[N]) {
    for (size_t i = 0; i < N; ++i)
        if (overlap(out, out_bytes, in[i].p, in[i].bytes)) return (int)i;
    return -1;
}

}  // namespace aesw_vanish

extern "C" {

int aesw_vanish_shape_ok(uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows) {
    return aesw::quot_shape_ok(aesw::QuotShape{k, ext_k, zeta_sel, n_sets, chunk_len, n_rows}) ? 1 : 0;
}

size_t aesw_vanish_tables_bytes(uint32_t k, uint32_t ext_k) { return (size_t)aesw::quot_tables_bytes(k, ext_k); }

size_t aesw_vanish_scalars_bytes(uint32_t n_sets, uint32_t chunk_len) { return (size_t)aesw::vanish_scalars_bytes(n_sets, chunk_len); }

size_t aesw_vanish_scalars_offset(uint32_t table, uint32_t index) {
    const uint64_t cell = aesw::vanish_table_at(table, index);
    return cell == ~(uint64_t)0 ? (size_t)-1 : (size_t)(cell * sizeof(aesw::Fr));
}

int aesw_vanish_tables_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint8_t *d_tables, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_tables_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!quot_k_ok(k, ext_k) || zeta_sel > 1) return refuse(ctx, call, "k must be 10 ... 28, ext_k k + 2 ... 28 and zeta_sel 0 or 1");
    if (bad_pointer(d_tables)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(vanish_tables_kernel, dim3((quot_tables(k, ext_k).cells + THREADS - 1) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       cells(d_tables), k, ext_k, zeta_sel);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vanish_scalars_device(aesw_ctx *ctx, uint32_t n_sets, uint32_t chunk_len, const uint8_t *d_theta, const uint8_t *d_beta, const uint8_t *d_gamma,
                               const uint8_t *d_y, uint8_t *d_scalars, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_scalars_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!quot_sets_ok(n_sets) || !sigma_chunk_len_ok(chunk_len)) return refuse(ctx, call, "n_sets must be 1 ... 1024 and chunk_len 1 ... 8");
    if (bad_pointer(d_theta)) return refuse(ctx, call, "d_theta must be there and 16-byte aligned");
    if (bad_pointer(d_beta)) return refuse(ctx, call, "d_beta must be there and 16-byte aligned");
    if (bad_pointer(d_gamma)) return refuse(ctx, call, "d_gamma must be there and 16-byte aligned");
    if (bad_pointer(d_y)) return refuse(ctx, call, "d_y must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    const Input in[] = {{d_theta, sizeof(Fr)}, {d_beta, sizeof(Fr)}, {d_gamma, sizeof(Fr)}, {d_y, sizeof(Fr)}};
    if (first_overlap(d_scalars, vanish_scalars_bytes(n_sets, chunk_len), in) >= 0) return refuse(ctx, call, "d_scalars must not overlap d_theta, d_beta, d_gamma or d_y");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(vanish_scalars_kernel, dim3(1), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), cells(d_theta), cells(d_beta), cells(d_gamma), cells(d_y),
                       cells(d_scalars), n_sets, chunk_len);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vanish_head_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, const uint8_t *d_words,
                            const uint8_t *d_rcon, const uint8_t *d_zperm, const uint8_t *d_l, const uint8_t *d_scalars, uint8_t *d_acc_out, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_head_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    const QuotShape q{k, ext_k, 0u, n_sets, chunk_len, n_rows};
    if (!quot_shape_ok(q)) return refuse(ctx, call, SHAPE);
    if (bad_pointer(d_words)) return refuse(ctx, call, "d_words must be there and 16-byte aligned");
    if (bad_pointer(d_rcon)) return refuse(ctx, call, "d_rcon must be there and 16-byte aligned");
    if (bad_pointer(d_zperm)) return refuse(ctx, call, "d_zperm must be there and 16-byte aligned");
    if (bad_pointer(d_l)) return refuse(ctx, call, "d_l must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_acc_out)) return refuse(ctx, call, "d_acc_out must be there and 16-byte aligned");
    const Input in[] = {{d_words, group_bytes(ext_k, 1)}, {d_rcon, group_bytes(ext_k, 2)}, {d_zperm, group_bytes(ext_k, quot_perm_sets(n_sets, chunk_len))},
                        {d_l, group_bytes(ext_k, 3)}, {d_scalars, vanish_scalars_bytes(n_sets, chunk_len)}};
    if (first_overlap(d_acc_out, group_bytes(ext_k, 1), in) >= 0) return refuse(ctx, call, "d_acc_out must not overlap d_words, d_rcon, d_zperm, d_l or d_scalars");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const HeadParams p{cells(d_words), cells(d_rcon), cells(d_zperm), cells(d_l), cells(d_scalars), cells(d_acc_out), q};
    with_nt((int)ctx->opt.fr_nt, [&](auto n) {
        hipLaunchKernelGGL(vanish_head_kernel<AESW_V(n)>, dim3((1u << ext_k) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vanish_perm_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, uint32_t set, const uint8_t *d_values,
                            const uint8_t *d_sigma, const uint8_t *d_z, const uint8_t *d_l, const uint8_t *d_tables, const uint8_t *d_scalars, const uint8_t *d_acc_in,
                            uint8_t *d_acc_out, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_perm_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    const QuotShape q{k, ext_k, 0u, n_sets, chunk_len, n_rows};
    if (!quot_shape_ok(q)) return refuse(ctx, call, SHAPE);
    if (set >= quot_perm_sets(n_sets, chunk_len)) return refuse(ctx, call, "set must be below the number of permutation sets");
    if (bad_pointer(d_values)) return refuse(ctx, call, "d_values must be there and 16-byte aligned");
    if (bad_pointer(d_sigma)) return refuse(ctx, call, "d_sigma must be there and 16-byte aligned");
    if (bad_pointer(d_z)) return refuse(ctx, call, "d_z must be there and 16-byte aligned");
    if (bad_pointer(d_l)) return refuse(ctx, call, "d_l must be there and 16-byte aligned");
    if (bad_pointer(d_tables)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_acc_in)) return refuse(ctx, call, "d_acc_in must be there and 16-byte aligned");
    if (bad_pointer(d_acc_out)) return refuse(ctx, call, "d_acc_out must be there and 16-byte aligned");
    const uint32_t columns = sigma_set_end(set, chunk_len, sigma_columns(n_sets)) - sigma_set_first(set, chunk_len);
    const uint64_t one = group_bytes(ext_k, 1);
    const Input in[] = {{d_values, group_bytes(ext_k, columns)}, {d_sigma, group_bytes(ext_k, columns)}, {d_z, one}, {d_l, group_bytes(ext_k, 3)},
                        {d_tables, quot_tables_bytes(k, ext_k)}, {d_scalars, vanish_scalars_bytes(n_sets, chunk_len)}};
    if (first_overlap(d_acc_out, one, in) >= 0) return refuse(ctx, call, "d_acc_out must not overlap d_values, d_sigma, d_z, d_l, d_tables or d_scalars");
    if (d_acc_in != d_acc_out && overlap(d_acc_in, one, d_acc_out, one)) return refuse(ctx, call, "d_acc_in must be d_acc_out itself or must not overlap it");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const PermParams p{cells(d_values), cells(d_sigma), cells(d_z), cells(d_l), cells(d_tables), cells(d_scalars), cells(d_acc_in), cells(d_acc_out), q, set};
    with_nt((int)ctx->opt.fr_nt, [&](auto n) {
        hipLaunchKernelGGL(vanish_perm_kernel<AESW_V(n)>, dim3((1u << ext_k) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vanish_lookup_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, uint32_t set, const uint8_t *d_advice3,
                              const uint8_t *d_selectors5, const uint8_t *d_table4, const uint8_t *d_a5, const uint8_t *d_s5, const uint8_t *d_z5, const uint8_t *d_l,
                              const uint8_t *d_scalars, const uint8_t *d_acc_in, uint8_t *d_acc_out, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_lookup_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    const QuotShape q{k, ext_k, 0u, n_sets, chunk_len, n_rows};
    if (!quot_shape_ok(q)) return refuse(ctx, call, SHAPE);
    if (set >= n_sets) return refuse(ctx, call, "set must be below n_sets");
    if (bad_pointer(d_advice3)) return refuse(ctx, call, "d_advice3 must be there and 16-byte aligned");
    if (bad_pointer(d_selectors5)) return refuse(ctx, call, "d_selectors5 must be there and 16-byte aligned");
    if (bad_pointer(d_table4)) return refuse(ctx, call, "d_table4 must be there and 16-byte aligned");
    if (bad_pointer(d_a5)) return refuse(ctx, call, "d_a5 must be there and 16-byte aligned");
    if (bad_pointer(d_s5)) return refuse(ctx, call, "d_s5 must be there and 16-byte aligned");
    if (bad_pointer(d_z5)) return refuse(ctx, call, "d_z5 must be there and 16-byte aligned");
    if (bad_pointer(d_l)) return refuse(ctx, call, "d_l must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_acc_in)) return refuse(ctx, call, "d_acc_in must be there and 16-byte aligned");
    if (bad_pointer(d_acc_out)) return refuse(ctx, call, "d_acc_out must be there and 16-byte aligned");
    const uint64_t one = group_bytes(ext_k, 1), five = group_bytes(ext_k, THETA_TAGS);
    const Input in[] = {{d_advice3, group_bytes(ext_k, 3)}, {d_selectors5, five}, {d_table4, group_bytes(ext_k, 4)}, {d_a5, five}, {d_s5, five}, {d_z5, five},
                        {d_l, group_bytes(ext_k, 3)}, {d_scalars, vanish_scalars_bytes(n_sets, chunk_len)}};
    if (first_overlap(d_acc_out, one, in) >= 0)
        return refuse(ctx, call, "d_acc_out must not overlap d_advice3, d_selectors5, d_table4, d_a5, d_s5, d_z5, d_l or d_scalars");
    if (d_acc_in != d_acc_out && overlap(d_acc_in, one, d_acc_out, one)) return refuse(ctx, call, "d_acc_in must be d_acc_out itself or must not overlap it");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const LookupParams p{cells(d_advice3), cells(d_selectors5), cells(d_table4), cells(d_a5), cells(d_s5), cells(d_z5), cells(d_l), cells(d_scalars),
                         cells(d_acc_in), cells(d_acc_out), q, set};
    with_nt((int)ctx->opt.fr_nt, [&](auto n) {
        hipLaunchKernelGGL(vanish_lookup_kernel<AESW_V(n)>, dim3((1u << ext_k) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vanish_divide_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, const uint8_t *d_tables, const uint8_t *d_acc_in, uint8_t *d_acc_out, void *stream) {
    using namespace aesw_vanish;
    const char *const call = "aesw_vanish_divide_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!quot_k_ok(k, ext_k)) return refuse(ctx, call, "k must be 10 ... 28 and ext_k k + 2 ... 28");
    if (bad_pointer(d_tables)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    if (bad_pointer(d_acc_in)) return refuse(ctx, call, "d_acc_in must be there and 16-byte aligned");
    if (bad_pointer(d_acc_out)) return refuse(ctx, call, "d_acc_out must be there and 16-byte aligned");
    const uint64_t one = group_bytes(ext_k, 1);
    if (overlap(d_acc_out, one, d_tables, quot_tables_bytes(k, ext_k))) return refuse(ctx, call, "d_acc_out must not overlap d_tables");
    if (d_acc_in != d_acc_out && overlap(d_acc_in, one, d_acc_out, one)) return refuse(ctx, call, "d_acc_in must be d_acc_out itself or must not overlap it");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    with_nt((int)ctx->opt.fr_nt, [&](auto n) {
        hipLaunchKernelGGL(vanish_divide_kernel<AESW_V(n)>, dim3((1u << ext_k) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), cells(d_tables),
                           cells(d_acc_in), cells(d_acc_out), k, ext_k);
    });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
