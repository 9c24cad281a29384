// shplonk/aesw_shplonk.hip -- libaesw_shplonk.so (include/aesw_shplonk.h): SHPLONK's multi-opening argument over coefficient
// columns, on the device.  The field is aesw_fr.h's; the chunks, the turns, the power indices, the workspace
// and open_join are aesw_open.h's; the plan, the scalars block, the report and what a thread of the small phases and a lane of
// the scan pass compute are aesw_shplonk.h's; nothing of the three is restated here.  What is here:
//   * shplonk_prepare_kernel, one workgroup: the plan, y^j, v^i, and per (set, point) e_is, w_is and v^i w_is; then per set -R_i
//     through LDS; the report reset;
//   * shplonk_finish_kernel, one wave: z_i, z_T, z_0^-1, the coefficients of L', its constant and its low cells;
//   * shplonk_combine_kernel<NT>: a lane per cell, acc + sum_j coefs[j] col_j (+ a low cell);
//   * shplonk_powers_kernel, shplonk_chunk_kernel, shplonk_carry_kernel: the powers of a set's points, the numerator's chunks at
//     every point of the set over one read, and every chunk's carry-in per point -- aesw_open.hip's passes with the set's t
//     points read from the plan in the scalars block.  open_wave_suffix and lane_cells are restated from aesw_open.hip: moved
//     into aesw_open.h they would make that header device code, which tests/test_open_model.py compiles with g++;
//   * shplonk_scan_kernel<NT>: per point the lane's Horner, the wave's suffix scan, the join from the chunk's carry-in and
//     S^(s) behind each of the lane's four cells, times v^i w_is, accumulated in registers; one 128-byte store a lane;
//   * shplonk_report_kernel: the remainders folded into the report;
//   * the entry points and their checks.
// No atomic and nothing to reset but the report: the passes are ordered by the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_shplonk.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_open.h"
#include "../aesw_shplonk.h"

namespace aesw_shplonk {
using namespace aesw;

constexpr int THREADS = OPEN_THREADS, ROWS = OPEN_ROWS_PER_LANE, WAVES = OPEN_WAVES;
constexpr uint32_t SETS = SHPLONK_MAX_SETS, SET_POINTS = SHPLONK_MAX_SET_POINTS;
static_assert(sizeof(Fr) == 32 && OPEN_LANES == LANES && SETS * SET_POINTS <= THREADS && SHPLONK_PLAN_WORDS == THREADS,
              "a thread of the prepare kernel per plan word and per (set, point)");

// a word of the plan at the front of the scalars block
__device__ __forceinline__ uint32_t plan_word(const u32x4 *scalars, uint32_t i) { return reinterpret_cast<const uint32_t *>(scalars)[i]; }
__device__ __forceinline__ uint32_t plan_sets(const u32x4 *scalars) { return shplonk_clamp(plan_word(scalars, SHPLONK_PLAN_N_SETS), SETS); }
__device__ __forceinline__ uint32_t plan_t(const u32x4 *scalars, uint32_t set) { return shplonk_clamp(plan_word(scalars, SHPLONK_PLAN_T + set), SET_POINTS); }
// the super-set index of point s of a set: below 16 whatever the block holds
__device__ __forceinline__ uint32_t plan_index(const u32x4 *scalars, uint32_t set, uint32_t s) {
    return plan_word(scalars, SHPLONK_PLAN_INDEX + SET_POINTS * set + s) & (SHPLONK_MAX_POINTS - 1);
}

// ---- the small phases -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(THREADS) shplonk_prepare_kernel(const ShplonkPlan plan, const u32x4 *__restrict__ points, const u32x4 *__restrict__ evals,
                                                                   const u32x4 *__restrict__ y_cell, const u32x4 *__restrict__ v_cell, u32x4 *__restrict__ scalars,
                                                                   uint64_t *__restrict__ report) {
    __shared__ Fr s_scaled[SETS][SET_POINTS];  // e_is w_is
    __shared__ Fr s_z[SETS][SET_POINTS + 1];   // Z_i(X)
    __shared__ Fr s_out[SETS][SET_POINTS];     // -R_i(X)
    __shared__ uint32_t s_zero[SETS * SET_POINTS];
    const uint32_t tid = threadIdx.x, n_sets = plan.w[SHPLONK_PLAN_N_SETS], max_cols = plan.w[SHPLONK_PLAN_MAX_COLS];
    reinterpret_cast<uint32_t *>(scalars)[tid] = plan.w[tid];
    const Fr y = load_cell(y_cell), v = load_cell(v_cell);
#pragma unroll 1
    for (uint32_t j = tid; j < max_cols; j += THREADS) store_cell<0>(cell_at(scalars, SHPLONK_AT_Y_POW + j), shplonk_pow(y, j));
    if (tid < SETS) store_cell<0>(cell_at(scalars, SHPLONK_AT_V_POW + tid), tid < n_sets ? shplonk_pow(v, tid) : FR_ZERO);
    if (tid < SETS * SET_POINTS) {
        const uint32_t i = tid / SET_POINTS, s = tid % SET_POINTS, t = i < n_sets ? plan.w[SHPLONK_PLAN_T + i] : 0u;
        Fr ebar = FR_ZERO, w = FR_ZERO, vw = FR_ZERO;
        uint32_t zero = 0;
        if (s < t) {
            const uint32_t m = plan.w[SHPLONK_PLAN_M + i];
            const u32x4 *mine = cell_at(evals, (uint64_t)plan.w[SHPLONK_PLAN_EVAL + i] + s);
            ebar = shplonk_horner(m, y, [&](uint32_t j) { return load_cell(cell_at(mine, (uint64_t)j * t)); });
            w = shplonk_weight(t, s, [&](uint32_t r) { return load_cell(cell_at(points, plan.w[SHPLONK_PLAN_INDEX + SET_POINTS * i + r])); }, zero);
            vw = fr_mul(shplonk_pow(v, i), w);
        }
        s_scaled[i][s] = fr_mul(ebar, w);
        s_zero[tid] = zero;
        store_cell<0>(cell_at(scalars, SHPLONK_AT_EBAR + tid), ebar);
        store_cell<0>(cell_at(scalars, SHPLONK_AT_W + tid), w);
        store_cell<0>(cell_at(scalars, SHPLONK_AT_VW + tid), vw);
    }
    __syncthreads();
    if (tid < SETS) {  // thread i interpolates set i
        const uint32_t i = tid, t = i < n_sets ? plan.w[SHPLONK_PLAN_T + i] : 0u;
        shplonk_neg_interpolant(
            t, [&](uint32_t r) { return load_cell(cell_at(points, plan.w[SHPLONK_PLAN_INDEX + SET_POINTS * i + r])); }, [&](uint32_t s) { return s_scaled[i][s]; },
            [&](uint32_t r) -> Fr & { return s_z[i][r]; }, [&](uint32_t d) -> Fr & { return s_out[i][d]; });
#pragma unroll 1
        for (uint32_t d = 0; d < SET_POINTS; ++d) store_cell<0>(cell_at(scalars, SHPLONK_AT_NEG_R + SET_POINTS * i + d), d < t ? s_out[i][d] : FR_ZERO);
    }
    if (tid == 0) {
        uint64_t zeros = 0;
        for (uint32_t p = 0; p < SETS * SET_POINTS; ++p) zeros += s_zero[p];
        for (uint32_t word = 0; word < SHPLONK_REPORT_WORDS; ++word) report[word] = (SHPLONK_REP_NONE_MASK >> word & 1u) ? ~0ull : 0ull;
        report[SHPLONK_REP_ZERO_DIFFS] = zeros;
    }
}

// one wave: thread i < S works for set i, thread S for z_T and the coefficient of h
__global__ void __launch_bounds__(LANES) shplonk_finish_kernel(const u32x4 *__restrict__ points, const u32x4 *__restrict__ u_cell, u32x4 *__restrict__ scalars,
                                                                uint64_t *__restrict__ report) {
    __shared__ Fr s_coef[SETS + 1], s_term[SETS], s_z0_inv;
    const uint32_t tid = threadIdx.x, n_sets = plan_sets(scalars), n_points = shplonk_clamp(plan_word(scalars, SHPLONK_PLAN_N_POINTS), SHPLONK_MAX_POINTS);
    const uint32_t t = tid < n_sets ? plan_t(scalars, tid) : 0u;
    const Fr u = load_cell(u_cell);
    Fr z = FR_ZERO, r_u = FR_ZERO;
    if (tid <= n_sets) z = shplonk_vanish(n_points, tid < n_sets ? plan_word(scalars, SHPLONK_PLAN_MASK + tid) : 0u, u, [&](uint32_t p) { return load_cell(cell_at(points, p)); });
    if (tid < n_sets)  // R_i(u) = -(-R_i)(u)
        r_u = fr_sub(FR_ZERO, shplonk_horner(t, u, [&](uint32_t d) { return load_cell(cell_at(scalars, SHPLONK_AT_NEG_R + SET_POINTS * tid + d)); }));
    if (tid == 0) {
        const Fr inv = fr_inv(z);
        s_z0_inv = inv;
        store_cell<0>(cell_at(scalars, SHPLONK_AT_Z0_INV), inv);
        report[SHPLONK_REP_Z0_ZERO] = fr_is_zero(z) ? 1ull : 0ull;
    }
    __syncthreads();
    if (tid <= SETS) {
        Fr coef = FR_ZERO;
        if (tid <= n_sets) coef = fr_mul(s_z0_inv, z);
        if (tid < n_sets) coef = fr_mul(coef, load_cell(cell_at(scalars, SHPLONK_AT_V_POW + tid)));
        if (tid == n_sets) coef = fr_sub(FR_ZERO, coef);
        s_coef[tid] = coef;
        store_cell<0>(cell_at(scalars, SHPLONK_AT_L_COEF + tid), coef);
        if (tid < SETS) {
            s_term[tid] = fr_mul(coef, r_u);  // 0 from set n_sets on: r_u is
            store_cell<0>(cell_at(scalars, SHPLONK_AT_Z + tid), tid < n_sets ? z : FR_ZERO);
        }
        if (tid == n_sets) store_cell<0>(cell_at(scalars, SHPLONK_AT_Z_T), z);
    }
    __syncthreads();
    if (tid < SHPLONK_MAX_LOW) {  // thread d: cell d of the low cells; thread 0 the constant as well
        Fr low = FR_ZERO;
#pragma unroll 1
        for (uint32_t i = 0; i < n_sets; ++i) {
            const Fr term = fr_mul(s_coef[i], load_cell(cell_at(scalars, SHPLONK_AT_NEG_R + SET_POINTS * i + tid)));  // the cells from t_i on are 0
            low = fr_sub(low, term);
        }
        if (tid == 0) {
            Fr constant = FR_ZERO;
#pragma unroll 1
            for (uint32_t i = 0; i < n_sets; ++i) constant = fr_sub(constant, s_term[i]);
            store_cell<0>(cell_at(scalars, SHPLONK_AT_L_CONST), constant);
            low = fr_add(low, constant);
        }
        store_cell<0>(cell_at(scalars, SHPLONK_AT_L_LOW + tid), low);
    }
}

// ---- the combine ----------------------------------------------------------------------------------------------------------------

// grid: x = 256 cells.  acc_in may be out: a lane reads its cell before it writes it, and no other's.
template <int NT>
__global__ void __launch_bounds__(THREADS) shplonk_combine_kernel(const u32x4 *coeff, const u32x4 *coefs, const u32x4 *low, const u32x4 *acc_in, u32x4 *out, uint32_t k,
                                                                   uint32_t n_cols, uint32_t n_low) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;  // below 2^k: a column is whole workgroups
    Fr acc = FR_ZERO;
    if (acc_in) acc = load_cell(cell_at(acc_in, i));
    if (i < n_low) acc = fr_add(acc, load_cell(cell_at(low, i)));
    Fr next = load_cell(cell_at(coeff, i));
    acc = shplonk_combine_cell(
        acc, n_cols, [&](uint32_t j) { return load_cell(cell_at(coefs, j)); },
        [&](uint32_t j) {
            const Fr col = next;
            if (j + 1 < n_cols) next = load_cell(cell_at(coeff, ((uint64_t)(j + 1) << k) + i));  // the next column's cell is on its way during the product
            return col;
        });
    store_cell<NT>(cell_at(out, i), acc);
}

// ---- the quotient of a set --------------------------------------------------------------------------------------------------------

struct SetParams {
    const u32x4 *numer;    // [2^k] cells: N_i
    const u32x4 *points;   // the super set
    const u32x4 *scalars;  // the plan and v^i w_is
    const u32x4 *acc;      // [2^k] cells or null; may be out
    u32x4 *out;            // [2^k] cells; may be numer
    u32x4 *rem;            // [8] cells
    u32x4 *ws;             // the workspace: the powers of eight points, then their chunk cells
    uint32_t k, set;
};

// aesw_open.hip's: the inclusive suffix scan of one value per lane over a wave, additive and weighted
__device__ __forceinline__ Fr open_wave_suffix(Fr v, uint32_t lane, const u32x4 *powers, uint32_t base) {
#pragma unroll 1
    for (uint32_t j = 0; (1u << j) < (uint32_t)LANES; ++j) {
        const Fr other = shfl_down_cell(v, 1 << j);
        if (lane + (1u << j) < (uint32_t)LANES) v = open_join(v, load_cell(cell_at(powers, open_scan_power(base, j))), other);
    }
    return v;
}
// aesw_open.hip's: the lane's cells i0 ... i0 + ROWS - 1 of the column, 128 contiguous bytes
__device__ __forceinline__ void lane_cells(const u32x4 *column, uint32_t i0, Fr (&c)[ROWS]) {
    const u32x4 *at = cell_at(column, i0);
    fr_unrolled<ROWS>([&](auto q) { c[decltype(q)::value] = load_cell(cell_at(at, decltype(q)::value)); });
}

// one wave: thread s < t_i writes z_s^(2^e), e = 0 ... 28
__global__ void __launch_bounds__(LANES) shplonk_powers_kernel(const SetParams p) {
    if (threadIdx.x >= plan_t(p.scalars, p.set)) return;
    Fr z = load_cell(cell_at(p.points, plan_index(p.scalars, p.set, threadIdx.x)));
    u32x4 *out = cell_at(p.ws, open_power_at(threadIdx.x, 0));
#pragma unroll 1
    for (uint32_t e = 0; e < OPEN_POWERS; ++e) {
        store_cell<0>(cell_at(out, e), z);
        z = fr_mul(z, z);
    }
}

// grid: x = the chunk.  The cells are read once and stay in registers over the set's points; one LDS slot per point.
__global__ void __launch_bounds__(THREADS) shplonk_chunk_kernel(const SetParams p) {
    __shared__ Fr s_wave[SET_POINTS][WAVES];
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES, t = plan_t(p.scalars, p.set);
    Fr c[ROWS];
    lane_cells(p.numer, blockIdx.x * OPEN_CHUNK + threadIdx.x * ROWS, c);
#pragma unroll 1
    for (uint32_t pt = 0; pt < t; ++pt) {
        const u32x4 *powers = cell_at(p.ws, open_power_at(pt, 0));
        Fr h[ROWS];
        open_lane_horner(c, load_cell(cell_at(powers, OPEN_POWER_CELL)), h);
        const Fr total = open_wave_suffix(h[0], lane, powers, OPEN_POWER_LANE);
        if (lane == 0) s_wave[pt][wave] = total;
    }
    __syncthreads();
    if (threadIdx.x < t) {  // thread pt joins the four waves at point pt
        const uint32_t pt = threadIdx.x;
        const Fr v = open_join_waves<WAVES>(load_cell(cell_at(p.ws, open_power_at(pt, OPEN_POWER_WAVE))), FR_ZERO, [&](int w) { return s_wave[pt][w]; },
                                            [](int, const Fr &) {});
        store_cell<0>(cell_at(p.ws, open_chunk_at(p.k, SHPLONK_WS_POINTS, 0, pt, blockIdx.x)), v);
    }
}

// grid: x = the point, 8 workgroups of which t_i work.  aesw_open.hip's carry pass with the carries written: chunk c's cell becomes
// S at the first cell of chunk c + 1, in place, and rem[point] = N_i(z_point).
__global__ void __launch_bounds__(THREADS) shplonk_carry_kernel(const SetParams p) {
    __shared__ Fr s_wave[WAVES];
    const uint32_t pt = blockIdx.x, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES, chunks = open_chunks(p.k);
    if (pt >= plan_t(p.scalars, p.set)) return;  // the whole workgroup
    const u32x4 *powers = cell_at(p.ws, open_power_at(pt, 0));
    u32x4 *cells = cell_at(p.ws, open_chunk_at(p.k, SHPLONK_WS_POINTS, 0, pt, 0));
    const auto power = [&](uint32_t s) { return load_cell(cell_at(powers, s)); };
    const Fr weight = open_lane_weight(OPEN_POWER_CHUNK, lane, power);
    Fr running = FR_ZERO;  // the value of every chunk above this turn's, in every thread
#pragma unroll 1
    for (uint32_t turn = 0; turn < open_turns(p.k); ++turn) {
        const uint32_t i = open_turn_first(p.k, turn) + threadIdx.x;
        const Fr incl = open_wave_suffix(i < chunks ? load_cell(cell_at(cells, i)) : FR_ZERO, lane, powers, OPEN_POWER_CHUNK);
        if (lane == 0) s_wave[wave] = incl;
        __syncthreads();
        Fr above = FR_ZERO;  // the value above this wave
        running = open_join_waves<WAVES>(power(OPEN_POWER_CHUNK_WAVE), running, [&](int w) { return s_wave[w]; },
                                         [&](int w, const Fr &a) { if ((uint32_t)w == wave) above = a; });
        const Fr here = open_join(incl, weight, above);  // S at the first cell of chunk i
        Fr next = shfl_down_cell(here, 1);
        if (lane == LANES - 1) next = above;
        if (i < chunks) store_cell<0>(cell_at(cells, i), next);
        __syncthreads();  // s_wave is written again next turn
    }
    if (threadIdx.x == 0) store_cell<0>(cell_at(p.rem, pt), running);
}

// grid: x = the chunk.  A lane reads its 128 bytes of the numerator (and of acc) once, and writes 128 contiguous bytes once: the
// ones it read where out is numer or acc.
template <int NT>
__global__ void __launch_bounds__(THREADS) shplonk_scan_kernel(const SetParams p) {
    __shared__ Fr s_wave[SET_POINTS][WAVES];  // a slot per point: one barrier a point
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES, t = plan_t(p.scalars, p.set);
    const uint32_t i0 = blockIdx.x * OPEN_CHUNK + threadIdx.x * ROWS;
    Fr c[ROWS], o[ROWS];
    lane_cells(p.numer, i0, c);
    if (p.acc) {
        lane_cells(p.acc, i0, o);
    } else {
        fr_unrolled<ROWS>([&](auto at) { o[decltype(at)::value] = FR_ZERO; });
    }
#pragma unroll 1
    for (uint32_t pt = 0; pt < t; ++pt) {
        const u32x4 *powers = cell_at(p.ws, open_power_at(pt, 0));
        const auto power = [&](uint32_t s) { return load_cell(cell_at(powers, s)); };
        const Fr z = power(OPEN_POWER_CELL);
        Fr h[ROWS];
        open_lane_horner(c, z, h);
        const Fr incl = open_wave_suffix(h[0], lane, powers, OPEN_POWER_LANE);
        if (lane == 0) s_wave[pt][wave] = incl;
        const Fr weight = open_lane_weight(OPEN_POWER_LANE, lane, power);
        __syncthreads();
        Fr above = FR_ZERO;  // S at the first cell behind this wave; the carry-in: S at the first cell behind the chunk
        open_join_waves<WAVES>(power(OPEN_POWER_WAVE), load_cell(cell_at(p.ws, open_chunk_at(p.k, SHPLONK_WS_POINTS, 0, pt, blockIdx.x))),
                               [&](int w) { return s_wave[pt][w]; }, [&](int w, const Fr &a) { if ((uint32_t)w == wave) above = a; });
        const Fr here = open_join(incl, weight, above);  // S at i0
        Fr next = shfl_down_cell(here, 1);               // S at i0 + ROWS
        if (lane == LANES - 1) next = above;
        shplonk_lane_accumulate(c, z, next, load_cell(cell_at(p.scalars, SHPLONK_AT_VW + SET_POINTS * p.set + pt)), o);
    }
    u32x4 *out = cell_at(p.out, i0);
    fr_unrolled<ROWS>([&](auto at) { store_cell<NT>(cell_at(out, decltype(at)::value), o[decltype(at)::value]); });
}

// one wave: lane s < t_i looks at rem[s]; lane 0 adds the set to the report where one of them is not 0
__global__ void __launch_bounds__(LANES) shplonk_report_kernel(const SetParams p, uint64_t *__restrict__ report) {
    const bool bad = threadIdx.x < plan_t(p.scalars, p.set) && !fr_is_zero(load_cell(cell_at(p.rem, threadIdx.x)));
    const unsigned long long any = __ballot(bad);
    if (threadIdx.x == 0 && any) {
        report[SHPLONK_REP_BAD_SETS] += 1;
        if ((uint64_t)p.set < report[SHPLONK_REP_FIRST_BAD]) report[SHPLONK_REP_FIRST_BAD] = p.set;
    }
}

// ---- the checks -------------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }
inline uint64_t column_bytes(uint32_t k, uint32_t n_cols) { return ((uint64_t)n_cols << k) * sizeof(Fr); }
constexpr uint64_t BLOCK_FIXED_BYTES = (uint64_t)SHPLONK_AT_Y_POW * sizeof(Fr);  // of the scalars block, what every plan has

}  // namespace aesw_shplonk

extern "C" {

size_t aesw_shplonk_scalars_bytes(uint32_t n_sets, uint32_t max_cols) { return (size_t)aesw::shplonk_scalars_bytes(n_sets, max_cols); }

size_t aesw_shplonk_scalars_offset(uint32_t table, uint32_t set) {
    const uint64_t cell = aesw::shplonk_table_at(table, set);
    return cell == ~(uint64_t)0 ? (size_t)-1 : (size_t)(cell * sizeof(aesw::Fr));
}

size_t aesw_shplonk_workspace_bytes(uint32_t k) { return (size_t)aesw::shplonk_workspace_bytes(k); }

size_t aesw_shplonk_report_bytes(void) { return aesw::SHPLONK_REPORT_BYTES; }

int aesw_shplonk_prepare_device(aesw_ctx *ctx, uint32_t n_points, uint32_t n_sets, const uint32_t *set_points, const uint32_t *set_cols, const uint32_t *point_index,
                                const uint8_t *d_points, const uint8_t *d_evals, const uint8_t *d_y, const uint8_t *d_v, uint8_t *d_scalars, void *d_report, void *stream) {
    using namespace aesw_shplonk;
    const char *const call = "aesw_shplonk_prepare_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    ShplonkPlan plan;
    if (const char *why = shplonk_plan_fill(n_points, n_sets, set_points, set_cols, point_index, plan)) return refuse(ctx, call, why);
    if (bad_pointer(d_points)) return refuse(ctx, call, "d_points must be there and 16-byte aligned");
    if (bad_pointer(d_evals)) return refuse(ctx, call, "d_evals must be there and 16-byte aligned");
    if (bad_pointer(d_y)) return refuse(ctx, call, "d_y must be there and 16-byte aligned");
    if (bad_pointer(d_v)) return refuse(ctx, call, "d_v must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_report)) return refuse(ctx, call, "d_report must be there and 16-byte aligned");
    const uint64_t block = shplonk_scalars_bytes(n_sets, plan.w[SHPLONK_PLAN_MAX_COLS]), points_bytes = (uint64_t)n_points * sizeof(Fr),
                   evals_bytes = (uint64_t)shplonk_plan_evals(plan) * sizeof(Fr);
    if (overlap(d_scalars, block, d_points, points_bytes) || overlap(d_scalars, block, d_evals, evals_bytes) || overlap(d_scalars, block, d_y, sizeof(Fr)) ||
        overlap(d_scalars, block, d_v, sizeof(Fr)))
        return refuse(ctx, call, "d_scalars must not overlap d_points, d_evals, d_y or d_v");
    if (overlap(d_report, SHPLONK_REPORT_BYTES, d_scalars, block) || overlap(d_report, SHPLONK_REPORT_BYTES, d_points, points_bytes) ||
        overlap(d_report, SHPLONK_REPORT_BYTES, d_evals, evals_bytes) || overlap(d_report, SHPLONK_REPORT_BYTES, d_y, sizeof(Fr)) ||
        overlap(d_report, SHPLONK_REPORT_BYTES, d_v, sizeof(Fr)))
        return refuse(ctx, call, "d_report must not overlap d_scalars, d_points, d_evals, d_y or d_v");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(shplonk_prepare_kernel, dim3(1), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), plan, reinterpret_cast<const u32x4 *>(d_points),
                       reinterpret_cast<const u32x4 *>(d_evals), reinterpret_cast<const u32x4 *>(d_y), reinterpret_cast<const u32x4 *>(d_v),
                       reinterpret_cast<u32x4 *>(d_scalars), static_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_shplonk_finish_device(aesw_ctx *ctx, const uint8_t *d_points, const uint8_t *d_u, uint8_t *d_scalars, void *d_report, void *stream) {
    using namespace aesw_shplonk;
    const char *const call = "aesw_shplonk_finish_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (bad_pointer(d_points)) return refuse(ctx, call, "d_points must be there and 16-byte aligned");
    if (bad_pointer(d_u)) return refuse(ctx, call, "d_u must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (bad_pointer(d_report)) return refuse(ctx, call, "d_report must be there and 16-byte aligned");
    if (overlap(d_scalars, BLOCK_FIXED_BYTES, d_points, sizeof(Fr)) || overlap(d_scalars, BLOCK_FIXED_BYTES, d_u, sizeof(Fr)))
        return refuse(ctx, call, "d_scalars must not overlap d_points or d_u");
    if (overlap(d_report, SHPLONK_REPORT_BYTES, d_scalars, BLOCK_FIXED_BYTES) || overlap(d_report, SHPLONK_REPORT_BYTES, d_points, sizeof(Fr)) ||
        overlap(d_report, SHPLONK_REPORT_BYTES, d_u, sizeof(Fr)))
        return refuse(ctx, call, "d_report must not overlap d_scalars, d_points or d_u");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(shplonk_finish_kernel, dim3(1), dim3(LANES), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const u32x4 *>(d_points),
                       reinterpret_cast<const u32x4 *>(d_u), reinterpret_cast<u32x4 *>(d_scalars), static_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_shplonk_combine_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_coefs, const uint8_t *d_low, uint32_t n_low,
                                const uint8_t *d_acc_in, uint8_t *d_out, void *stream) {
    using namespace aesw_shplonk;
    const char *const call = "aesw_shplonk_combine_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!open_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (!open_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 65535");
    if (n_low > SHPLONK_MAX_LOW) return refuse(ctx, call, "n_low must be 0 ... 8");
    if (bad_pointer(d_coeff)) return refuse(ctx, call, "d_coeff must be there and 16-byte aligned");
    if (bad_pointer(d_coefs)) return refuse(ctx, call, "d_coefs must be there and 16-byte aligned");
    if (n_low ? bad_pointer(d_low) : d_low != nullptr) return refuse(ctx, call, "d_low must be there and 16-byte aligned, or NULL with n_low = 0");
    if (!aligned_to(d_acc_in, 16)) return refuse(ctx, call, "d_acc_in must be NULL or 16-byte aligned");
    if (bad_pointer(d_out)) return refuse(ctx, call, "d_out must be there and 16-byte aligned");
    const uint64_t coeff_bytes = column_bytes(k, n_cols), one = column_bytes(k, 1), coefs_bytes = (uint64_t)n_cols * sizeof(Fr), low_bytes = (uint64_t)n_low * sizeof(Fr);
    if (overlap(d_out, one, d_coeff, coeff_bytes) || overlap(d_out, one, d_coefs, coefs_bytes) || (n_low && overlap(d_out, one, d_low, low_bytes)))
        return refuse(ctx, call, "d_out must not overlap d_coeff, d_coefs or d_low");
    if (d_acc_in && d_acc_in != d_out && overlap(d_acc_in, one, d_out, one)) return refuse(ctx, call, "d_acc_in must be d_out itself or must not overlap it");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    with_nt((int)ctx->opt.fr_nt, [&](auto n) {
        hipLaunchKernelGGL(shplonk_combine_kernel<AESW_V(n)>, dim3((1u << k) / THREADS), dim3(THREADS), 0, s, reinterpret_cast<const u32x4 *>(d_coeff),
                           reinterpret_cast<const u32x4 *>(d_coefs), reinterpret_cast<const u32x4 *>(d_low), reinterpret_cast<const u32x4 *>(d_acc_in),
                           reinterpret_cast<u32x4 *>(d_out), k, n_cols, n_low);
    });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_shplonk_quotient_device(aesw_ctx *ctx, uint32_t k, uint32_t set, const uint8_t *d_numer, const uint8_t *d_points, const uint8_t *d_scalars,
                                 const uint8_t *d_acc_in, uint8_t *d_out, uint8_t *d_rem, void *d_workspace, void *d_report, void *stream) {
    using namespace aesw_shplonk;
    const char *const call = "aesw_shplonk_quotient_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!open_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28");
    if (set >= SHPLONK_MAX_SETS) return refuse(ctx, call, "set must be 0 ... 15");
    if (bad_pointer(d_numer)) return refuse(ctx, call, "d_numer must be there and 16-byte aligned");
    if (bad_pointer(d_points)) return refuse(ctx, call, "d_points must be there and 16-byte aligned");
    if (bad_pointer(d_scalars)) return refuse(ctx, call, "d_scalars must be there and 16-byte aligned");
    if (!aligned_to(d_acc_in, 16)) return refuse(ctx, call, "d_acc_in must be NULL or 16-byte aligned");
    if (bad_pointer(d_out)) return refuse(ctx, call, "d_out must be there and 16-byte aligned");
    if (bad_pointer(d_rem)) return refuse(ctx, call, "d_rem must be there and 16-byte aligned");
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    if (bad_pointer(d_report)) return refuse(ctx, call, "d_report must be there and 16-byte aligned");
    const uint64_t one = column_bytes(k, 1), rem_bytes = (uint64_t)SHPLONK_MAX_SET_POINTS * sizeof(Fr), ws_bytes = shplonk_workspace_bytes(k);
    if (d_out != d_numer && overlap(d_out, one, d_numer, one)) return refuse(ctx, call, "d_out must be d_numer itself or must not overlap it");
    if (d_acc_in && d_acc_in != d_out && overlap(d_acc_in, one, d_out, one)) return refuse(ctx, call, "d_acc_in must be d_out itself or must not overlap it");
    if (overlap(d_out, one, d_points, sizeof(Fr)) || overlap(d_out, one, d_scalars, BLOCK_FIXED_BYTES)) return refuse(ctx, call, "d_out must not overlap d_points or d_scalars");
    if (overlap(d_rem, rem_bytes, d_numer, one) || overlap(d_rem, rem_bytes, d_out, one) || (d_acc_in && overlap(d_rem, rem_bytes, d_acc_in, one)) ||
        overlap(d_rem, rem_bytes, d_points, sizeof(Fr)) || overlap(d_rem, rem_bytes, d_scalars, BLOCK_FIXED_BYTES))
        return refuse(ctx, call, "d_rem must not overlap d_numer, d_out, d_acc_in, d_points or d_scalars");
    if (overlap(d_workspace, ws_bytes, d_numer, one) || overlap(d_workspace, ws_bytes, d_out, one) || (d_acc_in && overlap(d_workspace, ws_bytes, d_acc_in, one)) ||
        overlap(d_workspace, ws_bytes, d_rem, rem_bytes) || overlap(d_workspace, ws_bytes, d_points, sizeof(Fr)) || overlap(d_workspace, ws_bytes, d_scalars, BLOCK_FIXED_BYTES))
        return refuse(ctx, call, "d_workspace must not overlap d_numer, d_out, d_acc_in, d_rem, d_points or d_scalars");
    if (overlap(d_report, SHPLONK_REPORT_BYTES, d_numer, one) || overlap(d_report, SHPLONK_REPORT_BYTES, d_out, one) ||
        (d_acc_in && overlap(d_report, SHPLONK_REPORT_BYTES, d_acc_in, one)) || overlap(d_report, SHPLONK_REPORT_BYTES, d_rem, rem_bytes) ||
        overlap(d_report, SHPLONK_REPORT_BYTES, d_workspace, ws_bytes) || overlap(d_report, SHPLONK_REPORT_BYTES, d_scalars, BLOCK_FIXED_BYTES))
        return refuse(ctx, call, "d_report must not overlap d_numer, d_out, d_acc_in, d_rem, d_workspace or d_scalars");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SetParams p{};
    p.numer = reinterpret_cast<const u32x4 *>(d_numer);
    p.points = reinterpret_cast<const u32x4 *>(d_points);
    p.scalars = reinterpret_cast<const u32x4 *>(d_scalars);
    p.acc = reinterpret_cast<const u32x4 *>(d_acc_in);
    p.out = reinterpret_cast<u32x4 *>(d_out);
    p.rem = reinterpret_cast<u32x4 *>(d_rem);
    p.ws = static_cast<u32x4 *>(d_workspace);
    p.k = k; p.set = set;
    const dim3 grid(open_chunks(k));  // <= 2^18
    hipLaunchKernelGGL(shplonk_powers_kernel, dim3(1), dim3(LANES), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(shplonk_chunk_kernel, grid, dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(shplonk_carry_kernel, dim3(SHPLONK_MAX_SET_POINTS), dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(shplonk_scan_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, p); });
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(shplonk_report_kernel, dim3(1), dim3(LANES), 0, s, p, static_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
