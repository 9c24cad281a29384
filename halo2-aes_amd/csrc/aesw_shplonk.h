// aesw_shplonk.h -- the rules of libaesw_shplonk.so, once: SHPLONK's multi-opening argument over coefficient
// columns.  It is halo2_proofs v0.3.0 poly/kzg/multiopen/shplonk/prover.rs restated from memory: parity with halo2 is NOT PINNED
// (no Rust toolchain here, as in aesw_open.h and aesw_transcript.h); what is pinned, exactly, is tests/shplonk_model.py.
// The argument itself -- that [h] and [W] open the columns' commitments to the claimed evaluations -- is held by
// tests/kzg_verifier.py, a verifier written from the other side of the paper that shares no rule with this header or that model;
// it holds neither halo2's transcript order nor its order of the point sets.
//
// A PLAN is static and made on the host: P distinct super-set points (cells in device memory), S sets; set i holds t_i strictly
// increasing indices into the super set and m_i columns.  With y, v, u cells in device memory and e_ijs the evaluation of column
// j of set i at the set's point s:
//   N^P_i(X) = sum_j y^j P_ij(X)                          e_is = sum_j y^j e_ijs
//   R_i(X)   the interpolant through (z_s, e_is): t_i coefficients, so N_i = N^P_i - R_i differs from N^P_i in its low t_i cells
//   Q_i      = N_i / prod_s (X - z_s) = sum_s w_is * kate(N_i, z_s),  w_is = 1 / prod_(r != s) (z_s - z_r)        (partial fractions)
//            exact whenever every N_i(z_s) = 0: w_is prod_(r != s) (X - z_r) are the Lagrange basis polynomials and they sum to 1
//   h(X)     = sum_i v^i Q_i(X)
//   z_i      = prod_(p not in set i) (u - p),  z_T = prod_p (u - p)
//   L(X)     = sum_i v^i z_i (N^P_i(X) - R_i(u)) - z_T h(X),   W(X) = z_0^-1 L(X) / (X - u), remainder 0
// kate(N, z) has the coefficients S_(i+1) of aesw_open.h's suffix recurrence, so Q_i is that scan run at the t_i points over one
// read of the cells, emitting sum_s w_is S^(s)_(i+1).  The chunks, the turns, the power indices, the workspace of one column at
// t points and open_join are aesw_open.h's, used as they are.
// Here: the bounds, the plan as 256 words, the scalars block and the report, and what one thread of the two small phases and one
// lane of the scan pass compute -- written once for the kernels of shplonk/aesw_shplonk.hip and for tests/shplonk_driver.cpp.
// No HIP call and no ROCm include: tests/test_shplonk_model.py compiles this header alone with g++.
#pragma once
#include <stdint.h>

#include "aesw_fr.h"
#include "aesw_open.h"

namespace aesw {

constexpr uint32_t SHPLONK_MAX_POINTS = OPEN_MAX_POINTS, SHPLONK_MAX_SETS = 16, SHPLONK_MAX_SET_POINTS = 8, SHPLONK_MAX_SET_COLS = OPEN_MAX_COLS;
constexpr uint32_t SHPLONK_MAX_LOW = SHPLONK_MAX_SET_POINTS;  // the low cells a combine adds: an interpolant has at most that many

// ---- the plan: 256 words, a kernel argument of the prepare kernel, which lays them at the front of the scalars block -----------
constexpr uint32_t SHPLONK_PLAN_WORDS = 256;
constexpr uint32_t SHPLONK_PLAN_N_POINTS = 0, SHPLONK_PLAN_N_SETS = 1, SHPLONK_PLAN_MAX_COLS = 2;
constexpr uint32_t SHPLONK_PLAN_T = 16;      // + i: t_i
constexpr uint32_t SHPLONK_PLAN_M = 32;      // + i: m_i
constexpr uint32_t SHPLONK_PLAN_MASK = 48;   // + i: bit p set where super-set point p is in set i
constexpr uint32_t SHPLONK_PLAN_EVAL = 64;   // + i: the first cell of set i in d_evals, sum over the sets before it of m t
constexpr uint32_t SHPLONK_PLAN_INDEX = 128; // + 8 i + s: the super-set index of point s of set i
struct ShplonkPlan {
    uint32_t w[SHPLONK_PLAN_WORDS];
};
static_assert(SHPLONK_PLAN_INDEX + SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS == SHPLONK_PLAN_WORDS && sizeof(ShplonkPlan) == 1024, "the plan is 32 cells");

// The plan from the host arrays of the ABI, or why it is refused.  point_index: the sets' indices one set behind the other.
inline const char *shplonk_plan_fill(uint32_t n_points, uint32_t n_sets, const uint32_t *set_points, const uint32_t *set_cols, const uint32_t *point_index, ShplonkPlan &plan) {
    for (uint32_t &w : plan.w) w = 0;
    if (n_points < 1 || n_points > SHPLONK_MAX_POINTS) return "n_points must be 1 ... 16";
    if (n_sets < 1 || n_sets > SHPLONK_MAX_SETS) return "n_sets must be 1 ... 16";
    if (!set_points || !set_cols || !point_index) return "set_points, set_cols and point_index must be there";
    plan.w[SHPLONK_PLAN_N_POINTS] = n_points;
    plan.w[SHPLONK_PLAN_N_SETS] = n_sets;
    uint32_t first = 0, evals = 0, max_cols = 0;
    for (uint32_t i = 0; i < n_sets; ++i) {
        const uint32_t t = set_points[i], m = set_cols[i];
        if (t < 1 || t > SHPLONK_MAX_SET_POINTS) return "set_points must be 1 ... 8 for every set";
        if (m < 1 || m > SHPLONK_MAX_SET_COLS) return "set_cols must be 1 ... 65535 for every set";
        for (uint32_t s = 0; s < t; ++s) {
            const uint32_t p = point_index[first + s];
            if (p >= n_points) return "point_index must be below n_points";
            if (s && p <= point_index[first + s - 1]) return "point_index must be strictly increasing within a set";
            plan.w[SHPLONK_PLAN_INDEX + SHPLONK_MAX_SET_POINTS * i + s] = p;
            plan.w[SHPLONK_PLAN_MASK + i] |= 1u << p;
        }
        plan.w[SHPLONK_PLAN_T + i] = t;
        plan.w[SHPLONK_PLAN_M + i] = m;
        plan.w[SHPLONK_PLAN_EVAL + i] = evals;
        first += t;
        evals += m * t;  // at most 16 * 65535 * 8
        max_cols = m > max_cols ? m : max_cols;
    }
    plan.w[SHPLONK_PLAN_MAX_COLS] = max_cols;
    return nullptr;
}
inline uint32_t shplonk_plan_evals(const ShplonkPlan &plan) {
    const uint32_t last = plan.w[SHPLONK_PLAN_N_SETS] - 1;
    return plan.w[SHPLONK_PLAN_EVAL + last] + plan.w[SHPLONK_PLAN_M + last] * plan.w[SHPLONK_PLAN_T + last];
}
// What a kernel that reads the plan back from the scalars block takes a word as: never past the tables, whatever the block holds.
AESW_MONT_HD constexpr uint32_t shplonk_clamp(uint32_t v, uint32_t most) { return v < most ? v : most; }

// ---- the scalars block, in cells: the plan, then the tables; those of a set are SHPLONK_MAX_SET_POINTS cells apart ---------------
constexpr uint32_t SHPLONK_AT_PLAN = 0;
constexpr uint32_t SHPLONK_AT_V_POW = SHPLONK_AT_PLAN + sizeof(ShplonkPlan) / sizeof(Fr);                      // [16]     v^i
constexpr uint32_t SHPLONK_AT_EBAR = SHPLONK_AT_V_POW + SHPLONK_MAX_SETS;                                       // [16][8]  e_is
constexpr uint32_t SHPLONK_AT_W = SHPLONK_AT_EBAR + SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS;                  // [16][8]  w_is
constexpr uint32_t SHPLONK_AT_VW = SHPLONK_AT_W + SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS;                    // [16][8]  v^i w_is
constexpr uint32_t SHPLONK_AT_NEG_R = SHPLONK_AT_VW + SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS;                // [16][8]  -R_i, t_i coefficients from the constant up
constexpr uint32_t SHPLONK_AT_Z = SHPLONK_AT_NEG_R + SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS;                 // [16]     z_i
constexpr uint32_t SHPLONK_AT_Z_T = SHPLONK_AT_Z + SHPLONK_MAX_SETS;                                            //          z_T
constexpr uint32_t SHPLONK_AT_Z0_INV = SHPLONK_AT_Z_T + 1;                                                      //          z_0^-1
constexpr uint32_t SHPLONK_AT_L_COEF = SHPLONK_AT_Z0_INV + 1;                                                   // [S + 1]  z_0^-1 v^i z_i, then -z_0^-1 z_T for h
constexpr uint32_t SHPLONK_AT_L_CONST = SHPLONK_AT_L_COEF + SHPLONK_MAX_SETS + 1;                               //          -z_0^-1 sum_i v^i z_i R_i(u)
constexpr uint32_t SHPLONK_AT_L_LOW = SHPLONK_AT_L_CONST + 1;  // [8]  z_0^-1 sum_i v^i z_i R_i(X), with the constant above added to its cell 0: the low cells of L' over the N_i
constexpr uint32_t SHPLONK_AT_Y_POW = SHPLONK_AT_L_LOW + SHPLONK_MAX_LOW;                                       // [max m]  y^j
constexpr uint32_t SHPLONK_TABLES = 13;  // the order above, SHPLONK_AT_PLAN first: the table ids of include/aesw_shplonk.h
constexpr bool shplonk_sets_ok(uint32_t n_sets) { return n_sets >= 1 && n_sets <= SHPLONK_MAX_SETS; }
constexpr bool shplonk_cols_ok(uint32_t m) { return m >= 1 && m <= SHPLONK_MAX_SET_COLS; }
constexpr bool shplonk_set_points_ok(uint32_t t) { return t >= 1 && t <= SHPLONK_MAX_SET_POINTS; }
constexpr uint64_t shplonk_scalars_bytes(uint32_t n_sets, uint32_t max_cols) {
    return shplonk_sets_ok(n_sets) && shplonk_cols_ok(max_cols) ? ((uint64_t)SHPLONK_AT_Y_POW + max_cols) * sizeof(Fr) : 0u;
}
// the cell of `table` (a table id) that belongs to set `set`, or ~0 for an id or a set there is none of
constexpr uint64_t shplonk_table_at(uint32_t table, uint32_t set) {
    constexpr uint32_t at[SHPLONK_TABLES] = {SHPLONK_AT_PLAN, SHPLONK_AT_V_POW, SHPLONK_AT_EBAR, SHPLONK_AT_W, SHPLONK_AT_VW, SHPLONK_AT_NEG_R, SHPLONK_AT_Z, SHPLONK_AT_Z_T,
                                             SHPLONK_AT_Z0_INV, SHPLONK_AT_L_COEF, SHPLONK_AT_L_CONST, SHPLONK_AT_L_LOW, SHPLONK_AT_Y_POW};
    constexpr uint32_t stride[SHPLONK_TABLES] = {0, 1, SHPLONK_MAX_SET_POINTS, SHPLONK_MAX_SET_POINTS, SHPLONK_MAX_SET_POINTS, SHPLONK_MAX_SET_POINTS, 1, 0, 0, 1, 0, 0, 0};
    if (table >= SHPLONK_TABLES || set > SHPLONK_MAX_SETS || (set == SHPLONK_MAX_SETS && at[table] != SHPLONK_AT_L_COEF) || (set && !stride[table])) return ~(uint64_t)0;
    return (uint64_t)at[table] + (uint64_t)stride[table] * set;
}
static_assert(SHPLONK_AT_V_POW == 32 && SHPLONK_AT_Y_POW == 604 && shplonk_scalars_bytes(1, 1) == 605 * 32 && shplonk_scalars_bytes(17, 1) == 0 && shplonk_scalars_bytes(1, 0) == 0 &&
                  shplonk_table_at(3, 2) == SHPLONK_AT_W + 16 && shplonk_table_at(9, 16) == SHPLONK_AT_L_COEF + 16 && shplonk_table_at(7, 1) == ~(uint64_t)0 &&
                  shplonk_table_at(13, 0) == ~(uint64_t)0,
              "the scalars block: 32 cells of plan, 572 of tables, then y^j");

// the workspace of a set's quotient: aesw_open.h's for one column at SHPLONK_MAX_SET_POINTS points (the powers of every point,
// then its chunk cells), whatever t_i is -- the entry point does not read the plan, which lies in device memory
constexpr uint32_t SHPLONK_WS_POINTS = SHPLONK_MAX_SET_POINTS;
constexpr uint64_t shplonk_workspace_bytes(uint32_t k) { return open_workspace_bytes(k, 1, SHPLONK_WS_POINTS); }
static_assert(shplonk_workspace_bytes(10) == (8 * 29 + 8) * 32 && shplonk_workspace_bytes(9) == 0, "29 powers and one cell per chunk for each of eight points");

// ---- the report: eight 64-bit words ---------------------------------------------------------------------------------------------
constexpr uint32_t SHPLONK_REPORT_WORDS = 8, SHPLONK_REPORT_BYTES = SHPLONK_REPORT_WORDS * 8;
constexpr uint32_t SHPLONK_REP_BAD_SETS = 0;    // sets with a remainder N_i(z_s) that is not 0: the evaluations do not belong to the columns
constexpr uint32_t SHPLONK_REP_FIRST_BAD = 1;   // the lowest such set, ~0 for none
constexpr uint32_t SHPLONK_REP_ZERO_DIFFS = 2;  // ordered pairs (s, r), r != s, of a set with z_s == z_r (fr_inv(0) = 0 stands for their weight)
constexpr uint32_t SHPLONK_REP_Z0_ZERO = 3;     // 1 where z_0 = 0: u is a super-set point outside set 0
constexpr uint32_t SHPLONK_REP_LAST_REM = 4;    // words 4 ... 7: the remainder of the last division as a cell -- d_rem of aesw_open_divide_device points here
constexpr uint32_t SHPLONK_REP_NONE_MASK = 1u << SHPLONK_REP_FIRST_BAD;

// ---- what a thread of the small phases computes ----------------------------------------------------------------------------------

// base^e, e < 2^17: square and multiply from the top by a loop that stays a loop
AESW_MONT_HD Fr shplonk_pow(const Fr &base, uint32_t e) {
    Fr r = FR_ONE;
    AESW_OPEN_ROLLED
    for (int b = 16; b >= 0; --b) {
        r = fr_mul(r, r);
        const Fr m = fr_mul(r, base);
        if (e >> b & 1u) r = m;
    }
    return r;
}

// sum_(j < m) y^j cell(j) by Horner from the last column down: e_is from the evaluations, R_i(u) from R_i's coefficients
template <class Cell>
AESW_MONT_HD Fr shplonk_horner(uint32_t m, const Fr &y, Cell &&cell) {
    Fr acc = FR_ZERO;
    AESW_OPEN_ROLLED
    for (uint32_t j = m; j-- > 0;) acc = fr_add(fr_mul(acc, y), cell(j));
    return acc;
}

// w_s = 1 / prod_(r != s) (z_s - z_r) over the t points point(r) of a set; zero_diffs counts the differences that are 0
template <class Point>
AESW_MONT_HD Fr shplonk_weight(uint32_t t, uint32_t s, Point &&point, uint32_t &zero_diffs) {
    const Fr zs = point(s);
    Fr prod = FR_ONE;
    AESW_OPEN_ROLLED
    for (uint32_t r = 0; r < t; ++r) {
        const Fr d = fr_sub(zs, point(r));
        const Fr m = fr_mul(prod, d);
        if (r != s) {
            prod = m;
            zero_diffs += fr_is_zero(d);
        }
    }
    return fr_inv(prod);
}

// -R(X) of a set, R the interpolant through (z_s, e_s): R = sum_s (e_s w_s) Z(X) / (X - z_s), Z = prod_r (X - z_r).  zcell(r),
// r = 0 ... t, and out(r), r < t, are cells the caller lends (LDS in the kernel): Z is built there, every quotient Z / (X - z_s)
// by synthetic division from the top, and out ends as the t coefficients of -R from the constant up.  The exact division needs
// no z_s to be distinct; where two are equal their weights are 0 and so is what they add.
template <class Point, class Scaled, class ZCell, class Out>
AESW_MONT_HD void shplonk_neg_interpolant(uint32_t t, Point &&point, Scaled &&scaled, ZCell &&zcell, Out &&out) {
    zcell(0) = FR_ONE;  // Z = 1, then times (X - z_r): the degree grows by one
    AESW_OPEN_ROLLED
    for (uint32_t r = 0; r < t; ++r) {
        const Fr z = point(r);
        zcell(r + 1) = zcell(r);
        AESW_OPEN_ROLLED
        for (uint32_t d = r; d > 0; --d) zcell(d) = fr_sub(zcell(d - 1), fr_mul(z, zcell(d)));
        zcell(0) = fr_sub(FR_ZERO, fr_mul(z, zcell(0)));
    }
    AESW_OPEN_ROLLED
    for (uint32_t d = 0; d < t; ++d) out(d) = FR_ZERO;
    AESW_OPEN_ROLLED
    for (uint32_t s = 0; s < t; ++s) {
        const Fr z = point(s), scale = scaled(s);
        Fr b = zcell(t);  // the quotient's coefficient d - 1 is b_d = Z_d + z b_(d+1), from the top
        AESW_OPEN_ROLLED
        for (uint32_t d = t; d > 0; --d) {
            out(d - 1) = fr_sub(out(d - 1), fr_mul(scale, b));
            b = fr_add(zcell(d - 1), fr_mul(z, b));
        }
    }
}

// prod over the super-set points p whose bit in `skip` is clear of (u - p): z_i with skip = the set's mask, z_T with skip = 0
template <class Point>
AESW_MONT_HD Fr shplonk_vanish(uint32_t n_points, uint32_t skip, const Fr &u, Point &&point) {
    Fr prod = FR_ONE;
    AESW_OPEN_ROLLED
    for (uint32_t p = 0; p < n_points; ++p) {
        const Fr m = fr_mul(prod, fr_sub(u, point(p)));
        if (!(skip >> p & 1u)) prod = m;
    }
    return prod;
}

// ---- what a lane of the scan pass adds for one point ---------------------------------------------------------------------------
// `above` = S at the cell behind the lane's last; o[j] += scale * S at the lane's cell j + 1 (open_lane_quotient's cells).  Seven products.
AESW_MONT_HD void shplonk_lane_accumulate(const Fr (&c)[OPEN_ROWS_PER_LANE], const Fr &z, const Fr &above, const Fr &scale, Fr (&o)[OPEN_ROWS_PER_LANE]) {
    Fr q[OPEN_ROWS_PER_LANE];
    open_lane_quotient(c, z, above, q);
    fr_unrolled<OPEN_ROWS_PER_LANE>([&](auto at) {
        constexpr int j = decltype(at)::value;
        o[j] = fr_add(o[j], fr_mul(scale, q[j]));
    });
}

// one cell of a combine: acc + sum_j coef(j) col(j), by a loop that stays a loop
template <class Coef, class Col>
AESW_MONT_HD Fr shplonk_combine_cell(const Fr &acc, uint32_t n_cols, Coef &&coef, Col &&col) {
    Fr out = acc;
    AESW_OPEN_ROLLED
    for (uint32_t j = 0; j < n_cols; ++j) out = fr_add(out, fr_mul(coef(j), col(j)));
    return out;
}

}  // namespace aesw
