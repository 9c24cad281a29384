// open/aesw_open.hip -- libaesw_open.so (include/aesw_open.h): coefficient columns evaluated at points, folded under v and
// divided by (X - z), on the device.  The field is aesw_fr.h's and the rules -- the suffix recurrence, the chunks
// and the turns, which power z^(2^s) joins which pieces, the workspace, the fold's order -- are aesw_open.h's; nothing of either
// is restated here.  What is here:
//   * open_powers_kernel: a thread squares its point 28 times into the workspace;
//   * open_chunk_kernel: a workgroup reads its chunk of one column once -- a lane its four cells, 128 bytes -- and, for every
//     point, folds it into one cell of the workspace: Horner in the lane, the additive suffix scan of the wave, the waves through LDS;
//   * open_carry_kernel: one workgroup per (column, point) scans the chunk cells from the last chunk down, 256 a turn, writes the
//     value of the column at the point and, for a division, every chunk's carry-in in place;
//   * open_scan_kernel<NT>: a workgroup makes the lane values of its chunk again and scans them down from its carry-in; a lane
//     stores its four cells of the quotient, 128 contiguous bytes, through aesw_store.h's flavour;
//   * open_fold_kernel<NT>: a lane folds its cell of every column under v;
//   * the entry points and the checks that are theirs alone.
// How a cell lies in memory and moves between lanes is aesw_fr_dev.h's; the scan of a wave here is additive and weighted, so it
// is this file's (open_wave_suffix).  No atomic, no look-back flag, nothing to reset: the passes are ordered by the stream and
// every output word is stored once per call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_open.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_open.h"

namespace aesw_open {
using namespace aesw;

constexpr int THREADS = OPEN_THREADS, ROWS = OPEN_ROWS_PER_LANE, WAVES = OPEN_WAVES;
static_assert(sizeof(Fr) == 32 && OPEN_LANES == LANES, "a cell is two 16-byte pieces; the rules count the lanes of a wave as the device does");

// Which launches the entry points enqueue: all of them, except in a measurement variant built with -DAESW_OPEN_PASSES=<mask>
// (tests/test_perf_open.py prices one kernel at a time that way; such a library's outputs are of no use).
#ifndef AESW_OPEN_PASSES
#define AESW_OPEN_PASSES 0x1f
#endif
constexpr unsigned PASSES = AESW_OPEN_PASSES, PASS_POWERS = 1, PASS_CHUNK = 2, PASS_CARRY = 4, PASS_SCAN = 8, PASS_FOLD = 16;

// ---- the powers ---------------------------------------------------------------------------------------------------------------

// one wave: thread p writes z_p^(2^s), s = 0 ... 28
__global__ void __launch_bounds__(LANES) open_powers_kernel(const u32x4 *__restrict__ points, u32x4 *__restrict__ ws, uint32_t n_points) {
    if (threadIdx.x >= n_points) return;
    Fr p = load_cell(cell_at(points, threadIdx.x));
    u32x4 *out = cell_at(ws, open_power_at(threadIdx.x, 0));
#pragma unroll 1
    for (uint32_t s = 0; s < OPEN_POWERS; ++s) {
        store_cell<0>(cell_at(out, s), p);
        p = fr_mul(p, p);
    }
}

// ---- a column at a point ------------------------------------------------------------------------------------------------------

// The inclusive suffix scan of one value per lane over a wave, additive and weighted: lane l ends with the value of the pieces of
// lanes l ... 63, a piece being 2^base cells long.  Every lane shuffles; the lanes that have a partner join.
__device__ __forceinline__ Fr open_wave_suffix(Fr v, uint32_t lane, const u32x4 *powers, uint32_t base) {
#pragma unroll 1
    for (uint32_t j = 0; (1u << j) < (uint32_t)LANES; ++j) {
        const Fr other = shfl_down_cell(v, 1 << j);
        if (lane + (1u << j) < (uint32_t)LANES) v = open_join(v, load_cell(cell_at(powers, open_scan_power(base, j))), other);
    }
    return v;
}

struct ColumnParams {
    const u32x4 *coeff;  // [n_cols][2^k] cells
    u32x4 *ws;           // the workspace: the powers, then the chunk cells
    u32x4 *quot;         // [n_cols][2^k] cells (the scan kernel); may be coeff
    uint32_t k, n_points;
};

// the lane's cells i0 ... i0 + ROWS - 1 of a column: 128 contiguous bytes
__device__ __forceinline__ void lane_cells(const ColumnParams &p, uint32_t column, uint32_t i0, Fr (&c)[ROWS]) {
    const u32x4 *at = cell_at(p.coeff, ((uint64_t)column << p.k) + i0);
    fr_unrolled<ROWS>([&](auto q) { c[decltype(q)::value] = load_cell(cell_at(at, decltype(q)::value)); });
}

// grid: x = the chunk, y = the column.  The cells are read once and stay in registers over the points.
__global__ void __launch_bounds__(THREADS) open_chunk_kernel(const ColumnParams p) {
    __shared__ Fr s_wave[OPEN_MAX_POINTS][WAVES];
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    Fr c[ROWS];
    lane_cells(p, blockIdx.y, blockIdx.x * OPEN_CHUNK + threadIdx.x * ROWS, c);
#pragma unroll 1
    for (uint32_t pt = 0; pt < p.n_points; ++pt) {
        const u32x4 *powers = cell_at(p.ws, open_power_at(pt, 0));
        Fr h[ROWS];
        open_lane_horner(c, load_cell(cell_at(powers, OPEN_POWER_CELL)), h);
        const Fr t = open_wave_suffix(h[0], lane, powers, OPEN_POWER_LANE);
        if (lane == 0) s_wave[pt][wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < p.n_points) {  // thread pt joins the four waves at point pt
        const uint32_t pt = threadIdx.x;
        const Fr v = open_join_waves<WAVES>(load_cell(cell_at(p.ws, open_power_at(pt, OPEN_POWER_WAVE))), FR_ZERO, [&](int w) { return s_wave[pt][w]; },
                                            [](int, const Fr &) {});
        store_cell<0>(cell_at(p.ws, open_chunk_at(p.k, p.n_points, blockIdx.y, pt, blockIdx.x)), v);
    }
}

// grid: x = column * n_points + point.  The chunk cells of the pair from the last chunk down, OPEN_TURN a turn; out[x] = the value
// of the column at the point.  write_carries: chunk i's cell becomes S at the first cell of chunk i + 1, in place -- a thread
// reads and writes its own cell alone.
__global__ void __launch_bounds__(THREADS) open_carry_kernel(u32x4 *__restrict__ ws, uint32_t k, uint32_t n_points, u32x4 *__restrict__ out, uint32_t write_carries) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t pt = blockIdx.x % n_points, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES, chunks = open_chunks(k);
    const u32x4 *powers = cell_at(ws, open_power_at(pt, 0));
    u32x4 *cells = cell_at(ws, open_chunk_at(k, n_points, blockIdx.x / n_points, pt, 0));
    const auto power = [&](uint32_t s) { return load_cell(cell_at(powers, s)); };
    Fr weight = FR_ZERO;  // of what lies above the wave, in this lane: the carries alone need it
    if (write_carries) weight = open_lane_weight(OPEN_POWER_CHUNK, lane, power);
    Fr running = FR_ZERO;  // the value of every chunk above this turn's, in every thread
#pragma unroll 1
    for (uint32_t t = 0; t < open_turns(k); ++t) {
        const uint32_t i = open_turn_first(k, t) + threadIdx.x;
        const Fr incl = open_wave_suffix(i < chunks ? load_cell(cell_at(cells, i)) : FR_ZERO, lane, powers, OPEN_POWER_CHUNK);
        if (lane == 0) s_wave[wave] = incl;
        __syncthreads();
        Fr above = FR_ZERO;  // the value above this wave
        running = open_join_waves<WAVES>(power(OPEN_POWER_CHUNK_WAVE), running, [&](int w) { return s_wave[w]; },
                                         [&](int w, const Fr &a) { if ((uint32_t)w == wave) above = a; });
        if (write_carries) {
            const Fr here = open_join(incl, weight, above);  // S at the first cell of chunk i
            Fr next = shfl_down_cell(here, 1);
            if (lane == LANES - 1) next = above;
            if (i < chunks) store_cell<0>(cell_at(cells, i), next);
        }
        __syncthreads();  // s_wave is written again next turn
    }
    if (threadIdx.x == 0) store_cell<0>(cell_at(out, blockIdx.x), running);
}

// grid: x = the chunk, y = the column; one point.  A lane writes 32 * ROWS contiguous bytes, the ones it read where quot is coeff.
template <int NT>
__global__ void __launch_bounds__(THREADS) open_scan_kernel(const ColumnParams p) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const uint32_t i0 = blockIdx.x * OPEN_CHUNK + threadIdx.x * ROWS;
    const u32x4 *powers = cell_at(p.ws, open_power_at(0, 0));
    const auto power = [&](uint32_t s) { return load_cell(cell_at(powers, s)); };
    Fr c[ROWS], h[ROWS];
    lane_cells(p, blockIdx.y, i0, c);
    const Fr z = power(OPEN_POWER_CELL);
    open_lane_horner(c, z, h);
    const Fr incl = open_wave_suffix(h[0], lane, powers, OPEN_POWER_LANE);
    if (lane == 0) s_wave[wave] = incl;
    const Fr weight = open_lane_weight(OPEN_POWER_LANE, lane, power);
    __syncthreads();
    Fr above = FR_ZERO;  // S at the first cell behind this wave; the carry-in: S at the first cell behind the chunk
    open_join_waves<WAVES>(power(OPEN_POWER_WAVE), load_cell(cell_at(p.ws, open_chunk_at(p.k, 1, blockIdx.y, 0, blockIdx.x))), [&](int w) { return s_wave[w]; },
                           [&](int w, const Fr &a) { if ((uint32_t)w == wave) above = a; });
    const Fr here = open_join(incl, weight, above);  // S at i0
    Fr next = shfl_down_cell(here, 1);               // S at i0 + ROWS
    if (lane == LANES - 1) next = above;
    Fr q[ROWS];
    open_lane_quotient(c, z, next, q);
    u32x4 *out = cell_at(p.quot, ((uint64_t)blockIdx.y << p.k) + i0);
    fr_unrolled<ROWS>([&](auto at) { store_cell<NT>(cell_at(out, decltype(at)::value), q[decltype(at)::value]); });
}

// ---- the fold -----------------------------------------------------------------------------------------------------------------

// grid: x = 256 cells.  acc_in may be folded: a lane reads its cell before it writes it, and no other's.
template <int NT>
__global__ void __launch_bounds__(THREADS) open_fold_kernel(const u32x4 *coeff, const u32x4 *v_cell, const u32x4 *acc_in, u32x4 *folded, uint32_t k, uint32_t n_cols) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;  // below 2^k: a column is whole workgroups
    const Fr v = load_cell(v_cell);
    Fr acc = FR_ZERO;
    if (acc_in) acc = load_cell(cell_at(acc_in, i));
    Fr next = load_cell(cell_at(coeff, i));
#pragma unroll 1
    for (uint32_t c = 0; c < n_cols; ++c) {
        const Fr col = next;
        if (c + 1 < n_cols) next = load_cell(cell_at(coeff, ((uint64_t)(c + 1) << k) + i));  // the next column's cell is on its way during the product
        acc = open_fold_step(acc, v, col);
    }
    store_cell<NT>(cell_at(folded, i), acc);
}

// ---- the checks ---------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }
inline uint64_t column_bytes(uint32_t k, uint32_t n_cols) { return ((uint64_t)n_cols << k) * sizeof(Fr); }

// what the three calls check of their shape alike, in this order
inline const char *bad_shape(uint32_t k, uint32_t n_cols) {
    if (!open_k_ok(k)) return "k must be 10 ... 28";
    if (!open_cols_ok(n_cols)) return "n_cols must be 1 ... 65535";
    return nullptr;
}

}  // namespace aesw_open

extern "C" {

size_t aesw_open_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t n_points) { return (size_t)aesw::open_workspace_bytes(k, n_cols, n_points); }

int aesw_open_evaluate_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t n_points, const uint8_t *d_coeff, const uint8_t *d_points, uint8_t *d_evals,
                              void *d_workspace, void *stream) {
    using namespace aesw_open;
    const char *const call = "aesw_open_evaluate_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_shape(k, n_cols)) return refuse(ctx, call, why);
    if (!open_points_ok(n_points)) return refuse(ctx, call, "n_points must be 1 ... 16");
    if (bad_pointer(d_coeff)) return refuse(ctx, call, "d_coeff must be there and 16-byte aligned");
    if (bad_pointer(d_points)) return refuse(ctx, call, "d_points must be there and 16-byte aligned");
    if (bad_pointer(d_evals)) return refuse(ctx, call, "d_evals must be there and 16-byte aligned");
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    const uint64_t coeff_bytes = column_bytes(k, n_cols), points_bytes = (uint64_t)n_points * sizeof(Fr), evals_bytes = (uint64_t)n_cols * points_bytes,
                   ws_bytes = open_workspace_bytes(k, n_cols, n_points);
    if (overlap(d_evals, evals_bytes, d_coeff, coeff_bytes) || overlap(d_evals, evals_bytes, d_points, points_bytes))
        return refuse(ctx, call, "d_evals must not overlap d_coeff or d_points");
    if (overlap(d_workspace, ws_bytes, d_evals, evals_bytes) || overlap(d_workspace, ws_bytes, d_coeff, coeff_bytes) || overlap(d_workspace, ws_bytes, d_points, points_bytes))
        return refuse(ctx, call, "d_workspace must not overlap d_evals, d_coeff or d_points");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ColumnParams p{};
    p.coeff = reinterpret_cast<const u32x4 *>(d_coeff);
    p.ws = static_cast<u32x4 *>(d_workspace);
    p.k = k; p.n_points = n_points;
    if constexpr (PASSES & PASS_POWERS) hipLaunchKernelGGL(open_powers_kernel, dim3(1), dim3(LANES), 0, s, reinterpret_cast<const u32x4 *>(d_points), p.ws, n_points);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CHUNK) hipLaunchKernelGGL(open_chunk_kernel, dim3(open_chunks(k), n_cols), dim3(THREADS), 0, s, p);  // <= 2^18 chunks, 65535 columns
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CARRY)
        hipLaunchKernelGGL(open_carry_kernel, dim3(n_cols * n_points), dim3(THREADS), 0, s, p.ws, k, n_points, reinterpret_cast<u32x4 *>(d_evals), 0u);  // < 2^20 pairs
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_open_fold_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_v, const uint8_t *d_acc_in, uint8_t *d_folded,
                          void *stream) {
    using namespace aesw_open;
    const char *const call = "aesw_open_fold_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_shape(k, n_cols)) return refuse(ctx, call, why);
    if (bad_pointer(d_coeff)) return refuse(ctx, call, "d_coeff must be there and 16-byte aligned");
    if (bad_pointer(d_v)) return refuse(ctx, call, "d_v must be there and 16-byte aligned");
    if (!aligned_to(d_acc_in, 16)) return refuse(ctx, call, "d_acc_in must be NULL or 16-byte aligned");
    if (bad_pointer(d_folded)) return refuse(ctx, call, "d_folded must be there and 16-byte aligned");
    const uint64_t coeff_bytes = column_bytes(k, n_cols), one = column_bytes(k, 1);
    if (overlap(d_folded, one, d_coeff, coeff_bytes) || overlap(d_folded, one, d_v, sizeof(Fr))) return refuse(ctx, call, "d_folded must not overlap d_coeff or d_v");
    if (d_acc_in && d_acc_in != d_folded && overlap(d_acc_in, one, d_folded, one)) return refuse(ctx, call, "d_acc_in must be d_folded itself or must not overlap it");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if constexpr (PASSES & PASS_FOLD)
        with_nt((int)ctx->opt.fr_nt, [&](auto n) {
            hipLaunchKernelGGL(open_fold_kernel<AESW_V(n)>, dim3((1u << k) / THREADS), dim3(THREADS), 0, s, reinterpret_cast<const u32x4 *>(d_coeff),
                               reinterpret_cast<const u32x4 *>(d_v), reinterpret_cast<const u32x4 *>(d_acc_in), reinterpret_cast<u32x4 *>(d_folded), k, n_cols);
        });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_open_divide_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_point, uint8_t *d_quot, uint8_t *d_rem,
                            void *d_workspace, void *stream) {
    using namespace aesw_open;
    const char *const call = "aesw_open_divide_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_shape(k, n_cols)) return refuse(ctx, call, why);
    if (bad_pointer(d_coeff)) return refuse(ctx, call, "d_coeff must be there and 16-byte aligned");
    if (bad_pointer(d_point)) return refuse(ctx, call, "d_point must be there and 16-byte aligned");
    if (bad_pointer(d_quot)) return refuse(ctx, call, "d_quot must be there and 16-byte aligned");
    if (bad_pointer(d_rem)) return refuse(ctx, call, "d_rem must be there and 16-byte aligned");
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    const uint64_t coeff_bytes = column_bytes(k, n_cols), rem_bytes = (uint64_t)n_cols * sizeof(Fr), ws_bytes = open_workspace_bytes(k, n_cols, 1);
    if (d_quot != d_coeff && overlap(d_quot, coeff_bytes, d_coeff, coeff_bytes)) return refuse(ctx, call, "d_quot must be d_coeff itself or must not overlap it");
    if (overlap(d_quot, coeff_bytes, d_point, sizeof(Fr))) return refuse(ctx, call, "d_quot must not overlap d_point");
    if (overlap(d_rem, rem_bytes, d_coeff, coeff_bytes) || overlap(d_rem, rem_bytes, d_quot, coeff_bytes) || overlap(d_rem, rem_bytes, d_point, sizeof(Fr)))
        return refuse(ctx, call, "d_rem must not overlap d_coeff, d_quot or d_point");
    if (overlap(d_workspace, ws_bytes, d_coeff, coeff_bytes) || overlap(d_workspace, ws_bytes, d_quot, coeff_bytes) || overlap(d_workspace, ws_bytes, d_rem, rem_bytes) ||
        overlap(d_workspace, ws_bytes, d_point, sizeof(Fr)))
        return refuse(ctx, call, "d_workspace must not overlap d_coeff, d_quot, d_rem or d_point");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ColumnParams p{};
    p.coeff = reinterpret_cast<const u32x4 *>(d_coeff);
    p.ws = static_cast<u32x4 *>(d_workspace);
    p.quot = reinterpret_cast<u32x4 *>(d_quot);
    p.k = k; p.n_points = 1;
    const dim3 grid(open_chunks(k), n_cols);
    if constexpr (PASSES & PASS_POWERS) hipLaunchKernelGGL(open_powers_kernel, dim3(1), dim3(LANES), 0, s, reinterpret_cast<const u32x4 *>(d_point), p.ws, 1u);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CHUNK) hipLaunchKernelGGL(open_chunk_kernel, grid, dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CARRY) hipLaunchKernelGGL(open_carry_kernel, dim3(n_cols), dim3(THREADS), 0, s, p.ws, k, 1u, reinterpret_cast<u32x4 *>(d_rem), 1u);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_SCAN) with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(open_scan_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, p); });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
