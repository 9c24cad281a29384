// aesw_vanish.h -- the rules of libaesw_vanish.so, once: the quotient h(X) of aesw_quot.h folded segment by
// segment.  The fold  acc = acc * y + constraint  is linear in acc, so it can be cut at any constraint boundary: a segment of
// `len` consecutive constraints is  acc_out[j] = acc_in[j] * y^len + seg(j),  seg the same fold started from 0.  Here: the
// segments of quot_numerator in its order, each written over the same `load(group, column, row)` of the caller's, so that the
// kernels of vanish/aesw_vanish.hip and the CPU driver of tests/vanish_driver.cpp run the same lines; the list of a shape's
// segments, their lengths, the field products each takes per row; and the scalars block, every value a segment needs that
// depends on the proof (theta, beta, gamma, y) and not on the row, derived once by a small kernel.
//   HEAD        the gate, l0 * (1 - Zp_0), l_last * (Zp_(S-1)^2 - Zp_(S-1)), the S - 1 chain constraints; it opens the fold
//   PERM(s)     the product constraint of permutation set s, from beta * delta^first(s) * x_j
//   LOOKUP(s)   the 25 constraints of column set s, five per tag; the inputs and the table under each arity once per row
//   DIVIDE      acc * vanish[j mod m]
// The bounds, the rotations, the tables, x_j and the column groups are aesw_quot.h's (quot_shape_ok, quot_rot, quot_tables,
// quot_table_cell, quot_point, QuotGroup); nothing of them is restated.  The constraint order and zeta are as little pinned
// against halo2 as they are there.
// No HIP call and no ROCm include: the tests compile this header alone with g++.
#pragma once
#include <stdint.h>

#include "aesw_quot.h"

namespace aesw {

// ---- the segments of a shape ------------------------------------------------------------------------------------------------------
enum VanishKind : uint32_t { VANISH_HEAD, VANISH_PERM, VANISH_LOOKUP, VANISH_DIVIDE, VANISH_KINDS };
struct VanishSegment {
    uint32_t kind, set;
};
constexpr uint32_t VANISH_LOOKUP_LEN = 5u * THETA_TAGS;  // five constraints per tag
AESW_QUOT_HD constexpr uint32_t vanish_segments(uint32_t n_sets, uint32_t chunk_len) { return 1u + quot_perm_sets(n_sets, chunk_len) + n_sets + 1u; }
// segment i of the fold: HEAD, PERM(0) ... PERM(S - 1), LOOKUP(0) ... LOOKUP(N - 1), DIVIDE
AESW_QUOT_HD constexpr VanishSegment vanish_segment(uint32_t n_sets, uint32_t chunk_len, uint32_t i) {
    const uint32_t sets = quot_perm_sets(n_sets, chunk_len);
    return i == 0 ? VanishSegment{VANISH_HEAD, 0u} : i <= sets ? VanishSegment{VANISH_PERM, i - 1u}
         : i <= sets + n_sets ? VanishSegment{VANISH_LOOKUP, i - 1u - sets} : VanishSegment{VANISH_DIVIDE, 0u};
}
// the constraints a segment of that kind folds (the division folds none)
AESW_QUOT_HD constexpr uint32_t vanish_segment_len(uint32_t kind, uint32_t n_sets, uint32_t chunk_len) {
    return kind == VANISH_HEAD ? 3u + (quot_perm_sets(n_sets, chunk_len) - 1u) : kind == VANISH_PERM ? 1u : kind == VANISH_LOOKUP ? VANISH_LOOKUP_LEN : 0u;
}
AESW_QUOT_HD constexpr uint32_t vanish_constraints(uint32_t n_sets, uint32_t chunk_len) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < vanish_segments(n_sets, chunk_len); ++i) sum += vanish_segment_len(vanish_segment(n_sets, chunk_len, i).kind, n_sets, chunk_len);
    return sum;
}
static_assert(vanish_segments(4, 3) == 11 && vanish_constraints(4, 3) == 1 + 2 + 4 + 5 + 100, "N = 4: the gate, 2 + (S - 1) + S of the permutation, 25 N of the lookups");

// The field products of a segment per row, in quot_products_per_row's own count: a segment's share of what quot_numerator takes, so
// that the shares sum to it exactly and a rate priced by them is priced as 4.23's was.  What the whole row shares -- x_j and
// beta * x_j; theta^2, theta^3 and the table under each arity -- is booked to the first segment that uses it, PERM(0) and LOOKUP(0).
AESW_QUOT_HD constexpr uint32_t vanish_segment_products(const VanishSegment &seg, uint32_t n_sets, uint32_t chunk_len) {
    const uint32_t cols = sigma_columns(n_sets), sets = sigma_sets(cols, chunk_len);
    if (seg.kind == VANISH_HEAD) return 1u + 2u + 3u + 2u * (sets - 1u);  // the gate; Zp_0 opens; Zp_(S-1) closes; the chain
    if (seg.kind == VANISH_PERM)  // per column beta * sigma, two running products, the next delta power; l_active and the fold; set 0: x_j, beta * x_j
        return 4u * (sigma_set_end(seg.set, chunk_len, cols) - sigma_set_first(seg.set, chunk_len)) + 2u + (seg.set == 0 ? 2u : 0u);
    if (seg.kind == VANISH_LOOKUP) return 2u + THETA_TAGS * 17u + (seg.set == 0 ? 5u : 0u);  // x_s, y_s, z_s under each arity; per argument 2 + 3 + 7 + 2 + 3
    return 1u;                                                                                // the division
}
AESW_QUOT_HD constexpr uint32_t vanish_products_per_row(uint32_t n_sets, uint32_t chunk_len) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < vanish_segments(n_sets, chunk_len); ++i) sum += vanish_segment_products(vanish_segment(n_sets, chunk_len, i), n_sets, chunk_len);
    return sum;
}
static_assert(vanish_products_per_row(1, 3) == quot_products_per_row(1, 3) && vanish_products_per_row(2, 2) == quot_products_per_row(2, 2) &&
              vanish_products_per_row(2, 3) == quot_products_per_row(2, 3) && vanish_products_per_row(4, 3) == quot_products_per_row(4, 3) &&
              vanish_products_per_row(8, 8) == quot_products_per_row(8, 8) && vanish_products_per_row(4, 3) == 436, "the segments' products sum to quot_products_per_row");
// What a call of the segment runs per row beyond (or below) its share, the price of the cut: every PERM call makes x_j and takes
// beta * delta^first(s) from the scalars block, and makes no power of delta behind its last column (4 c + 3 products in all);
// every LOOKUP call makes the table under each arity, and theta^2, theta^3 come from the block (90 in all).  S + 3 N - 7 a row.
AESW_QUOT_HD constexpr int32_t vanish_segment_overhead(const VanishSegment &seg) {
    return seg.kind == VANISH_PERM ? (seg.set == 0 ? -1 : 1) : seg.kind == VANISH_LOOKUP ? (seg.set == 0 ? -2 : 3) : 0;
}
AESW_QUOT_HD constexpr int32_t vanish_overhead_per_row(uint32_t n_sets, uint32_t chunk_len) {
    int32_t sum = 0;
    for (uint32_t i = 0; i < vanish_segments(n_sets, chunk_len); ++i) sum += vanish_segment_overhead(vanish_segment(n_sets, chunk_len, i));
    return sum;
}
static_assert(vanish_overhead_per_row(4, 3) == 5 + 12 - 7 && vanish_overhead_per_row(1, 3) == 2 + 3 - 7, "S + 3 N - 7: ten products on 436 at N = 4");

// ---- the scalars block, in cells ------------------------------------------------------------------------------------------------------
// Everything a segment needs that is per proof: the four challenges as they were when the scalars kernel ran, y^len per segment kind,
// theta^2 and theta^3, t * theta^(arity - 1) per tag, and per permutation set delta^first(s) with beta * delta^first(s) behind it.
enum VanishTable : uint32_t { VANISH_THETA, VANISH_BETA, VANISH_GAMMA, VANISH_Y, VANISH_Y_POW, VANISH_THETA_POW, VANISH_TAG, VANISH_DELTA, VANISH_BETA_DELTA, VANISH_TABLES };
constexpr uint32_t VANISH_AT_THETA = 0, VANISH_AT_BETA = 1, VANISH_AT_GAMMA = 2, VANISH_AT_Y = 3;
constexpr uint32_t VANISH_AT_Y_POW = 4;                                    // [3]     y^len of HEAD, PERM, LOOKUP
constexpr uint32_t VANISH_AT_THETA_POW = VANISH_AT_Y_POW + 3u;             // [2]     theta^2, theta^3
constexpr uint32_t VANISH_AT_TAG = VANISH_AT_THETA_POW + 2u;               // [5]     t * theta^(arity(t) - 1), t = 1 ... 5
constexpr uint32_t VANISH_AT_DELTA = VANISH_AT_TAG + THETA_TAGS;           // [S][2]  delta^first(s), beta * delta^first(s)
constexpr uint32_t VANISH_MAX_PERM_SETS = SIGMA_MAX_COLS;                  // chunk_len 1 at the most sets
AESW_QUOT_HD constexpr uint32_t vanish_scalars_cells(uint32_t n_sets, uint32_t chunk_len) { return VANISH_AT_DELTA + 2u * quot_perm_sets(n_sets, chunk_len); }
AESW_QUOT_HD constexpr uint64_t vanish_scalars_bytes(uint32_t n_sets, uint32_t chunk_len) {
    return quot_sets_ok(n_sets) && sigma_chunk_len_ok(chunk_len) ? (uint64_t)vanish_scalars_cells(n_sets, chunk_len) * sizeof(Fr) : 0u;
}
// the cell of entry `index` of `table`, or ~0 for a table or an entry there is none of
AESW_QUOT_HD constexpr uint64_t vanish_table_at(uint32_t table, uint32_t index) {
    return table <= VANISH_Y ? (index == 0 ? (uint64_t)table : ~(uint64_t)0)
         : table == VANISH_Y_POW ? (index < 3u ? (uint64_t)VANISH_AT_Y_POW + index : ~(uint64_t)0)
         : table == VANISH_THETA_POW ? (index < 2u ? (uint64_t)VANISH_AT_THETA_POW + index : ~(uint64_t)0)
         : table == VANISH_TAG ? (index < THETA_TAGS ? (uint64_t)VANISH_AT_TAG + index : ~(uint64_t)0)
         : table == VANISH_DELTA ? (index < VANISH_MAX_PERM_SETS ? (uint64_t)VANISH_AT_DELTA + 2u * index : ~(uint64_t)0)
         : table == VANISH_BETA_DELTA ? (index < VANISH_MAX_PERM_SETS ? (uint64_t)VANISH_AT_DELTA + 2u * index + 1u : ~(uint64_t)0) : ~(uint64_t)0;
}
static_assert(vanish_scalars_bytes(4, 3) == (14u + 10u) * 32u && vanish_table_at(VANISH_BETA_DELTA, 4) == 23 && vanish_table_at(VANISH_Y_POW, 3) == ~(uint64_t)0, "N = 4: 24 cells");
// cell `at` of the block, as the scalars kernel computes it
AESW_QUOT_HD Fr vanish_scalar_cell(uint32_t at, uint32_t n_sets, uint32_t chunk_len, const Fr &theta, const Fr &beta, const Fr &gamma, const Fr &y) {
    if (at == VANISH_AT_THETA) return theta;
    if (at == VANISH_AT_BETA) return beta;
    if (at == VANISH_AT_GAMMA) return gamma;
    if (at == VANISH_AT_Y) return y;
    if (at < VANISH_AT_THETA_POW) return fr_pow_u32(y, vanish_segment_len(at - VANISH_AT_Y_POW, n_sets, chunk_len));
    if (at < VANISH_AT_TAG) return fr_pow_u32(theta, at - VANISH_AT_THETA_POW + 2u);
    if (at < VANISH_AT_DELTA) {
        const uint32_t t = at - VANISH_AT_TAG + 1u;
        return quot_times_small(fr_pow_u32(theta, theta_arity(theta_table_of_tag(t)) - 1u), t);
    }
    const Fr power = fr_pow_u32(SIGMA_DELTA, sigma_set_first((at - VANISH_AT_DELTA) / 2u, chunk_len));
    return (at - VANISH_AT_DELTA) % 2u ? fr_mul(beta, power) : power;
}

// ---- the segments -----------------------------------------------------------------------------------------------------------------------
// load(group, column, row) is quot_numerator's, with one group more: VANISH_VALUES, column c of the permutation -- the advice
// column sigma_source_of_column names, or the fixed one behind them.  scalar(at) is cell `at` of the scalars block.  Every cell
// canonical.
constexpr uint32_t VANISH_VALUES = QUOT_GROUPS;
// which group and column of quot_numerator's a column of VANISH_VALUES is
AESW_QUOT_HD constexpr uint32_t vanish_values_group(uint32_t n_sets, uint32_t c) { return sigma_source_of_column(n_sets, c) <= 3u * n_sets ? QUOT_ADVICE : QUOT_RCON; }
AESW_QUOT_HD constexpr uint32_t vanish_values_column(uint32_t n_sets, uint32_t c) { return sigma_source_of_column(n_sets, c) <= 3u * n_sets ? sigma_source_of_column(n_sets, c) : 0u; }

// HEAD opens the fold: there is no acc_in
template <class Load, class Scalar>
AESW_QUOT_HD Fr vanish_head(const QuotShape &q, uint32_t j, Load &&load, Scalar &&scalar) {
    const uint32_t far = quot_rot(q.k, q.ext_k, j, (int32_t)q.n_rows), sets = quot_perm_sets(q.n_sets, q.chunk_len), words = 3u * q.n_sets;
    const Fr one = FR_ONE, y = scalar(VANISH_AT_Y), l0 = load(QUOT_L, 0, j);
    Fr acc = fr_mul(load(QUOT_RCON, 1, j), fr_sub(load(QUOT_ADVICE, words, j), load(QUOT_RCON, 0, j)));
    const auto fold = [&](const Fr &constraint) { acc = fr_add(fr_mul(acc, y), constraint); };
    fold(fr_mul(l0, fr_sub(one, load(QUOT_ZPERM, 0, j))));
    {
        const Fr z = load(QUOT_ZPERM, sets - 1, j);
        fold(fr_mul(load(QUOT_L, 1, j), fr_sub(fr_mul(z, z), z)));
    }
    AESW_QUOT_ROLLED
    for (uint32_t s = 1; s < sets; ++s) fold(fr_mul(l0, fr_sub(load(QUOT_ZPERM, s, j), load(QUOT_ZPERM, s - 1, far))));
    return acc;
}

// PERM(set): x = x_j
template <class Load, class Scalar>
AESW_QUOT_HD Fr vanish_perm(const QuotShape &q, uint32_t set, uint32_t j, const Fr &acc_in, const Fr &x, Load &&load, Scalar &&scalar) {
    const uint32_t next = quot_rot(q.k, q.ext_k, j, 1), cols = sigma_columns(q.n_sets);
    const uint32_t first = sigma_set_first(set, q.chunk_len), end = sigma_set_end(set, q.chunk_len, cols);
    const Fr beta = scalar(VANISH_AT_BETA), gamma = scalar(VANISH_AT_GAMMA), delta = SIGMA_DELTA;
    Fr bx = fr_mul(scalar((uint32_t)vanish_table_at(VANISH_BETA_DELTA, set)), x);  // beta * delta^c * x_j, column by column
    Fr left = load(QUOT_ZPERM, set, next), right = load(QUOT_ZPERM, set, j);
    AESW_QUOT_ROLLED
    for (uint32_t c = first; c < end; ++c) {
        const Fr vg = fr_add(load(VANISH_VALUES, c, j), gamma);
        left = fr_mul(left, fr_add(vg, fr_mul(beta, load(QUOT_SIGMA, c, j))));
        right = fr_mul(right, fr_add(vg, bx));
        if (c + 1u < end) bx = fr_mul(bx, delta);
    }
    return fr_add(fr_mul(acc_in, scalar(VANISH_AT_Y_POW + VANISH_PERM)), fr_mul(load(QUOT_L, 2, j), fr_sub(left, right)));
}

// LOOKUP(set): the fold runs on from acc_in, which is acc_in * y^25 + seg at no product more
template <class Load, class Scalar>
AESW_QUOT_HD Fr vanish_lookup(const QuotShape &q, uint32_t set, uint32_t j, const Fr &acc_in, Load &&load, Scalar &&scalar) {
    const uint32_t next = quot_rot(q.k, q.ext_k, j, 1), prev = quot_rot(q.k, q.ext_k, j, -1);
    const Fr one = FR_ONE, theta = scalar(VANISH_AT_THETA), beta = scalar(VANISH_AT_BETA), gamma = scalar(VANISH_AT_GAMMA), y = scalar(VANISH_AT_Y);
    const Fr l0 = load(QUOT_L, 0, j), l_last = load(QUOT_L, 1, j), l_active = load(QUOT_L, 2, j);
    Fr acc = acc_in;
    const auto fold = [&](const Fr &constraint) { acc = fr_add(fr_mul(acc, y), constraint); };
    const Fr tab2 = fr_add(fr_mul(load(QUOT_TABLE, 0, j), theta), load(QUOT_TABLE, 1, j));
    const Fr tab3 = fr_add(fr_mul(tab2, theta), load(QUOT_TABLE, 2, j));
    const Fr tab4 = fr_add(fr_mul(tab3, theta), load(QUOT_TABLE, 3, j));
    const Fr in2 = load(QUOT_ADVICE, 3u * set, j);
    const Fr in3 = fr_add(fr_mul(in2, theta), load(QUOT_ADVICE, 3u * set + 1u, j));
    const Fr in4 = fr_add(fr_mul(in3, theta), load(QUOT_ADVICE, 3u * set + 2u, j));
    AESW_QUOT_ROLLED
    for (uint32_t t = 1; t <= THETA_TAGS; ++t) {
        const uint32_t arity = theta_arity(theta_table_of_tag(t)), at = set * THETA_TAGS + t - 1u;
        const Fr in = fr_mul(load(QUOT_SELECTOR, at, j), fr_add(scalar(VANISH_AT_TAG + t - 1u), quot_pick(arity, in2, in3, in4)));
        const Fr z = load(QUOT_ZLOOKUP, at, j);
        fold(fr_mul(l0, fr_sub(one, z)));
        fold(fr_mul(l_last, fr_sub(fr_mul(z, z), z)));
        const Fr a = load(QUOT_A, at, j), sp = load(QUOT_S, at, j);
        const Fr left = fr_mul(fr_mul(load(QUOT_ZLOOKUP, at, next), fr_add(a, beta)), fr_add(sp, gamma));
        const Fr right = fr_mul(fr_mul(z, fr_add(in, beta)), fr_add(quot_pick(arity, tab2, tab3, tab4), gamma));
        fold(fr_mul(l_active, fr_sub(left, right)));
        const Fr d = fr_sub(a, sp);
        fold(fr_mul(l0, d));
        fold(fr_mul(fr_mul(l_active, d), fr_sub(a, load(QUOT_A, at, prev))));
    }
    return acc;
}

// DIVIDE: cell(at) is cell `at` of aesw_quot.h's tables
template <class Cell>
AESW_QUOT_HD Fr vanish_divide(uint32_t k, uint32_t ext_k, uint32_t j, const Fr &acc_in, Cell &&cell) {
    return fr_mul(acc_in, cell(quot_tables(k, ext_k).vanish_at + quot_vanish_index(k, ext_k, j)));
}

}  // namespace aesw
