// aesw_quot.h -- the rules of libaesw_quot.so, once: the quotient h(X) of a FixedAes128Config<k, n_sets> circuit on
// the extended coset, halo2's evaluate_h.  Here: the bounds, which row a rotation reads, which cell of the vanishing table a row
// takes, the tables, the label a cell index of sigma names, the order of the column groups, and the fold itself -- every
// constraint in its order, written over a `load(group, column, row)` of the caller's, so that a kernel and the CPU driver of
// tests/quot_driver.cpp run the same lines -- with the number of field products it takes per row.  Of these the label of sigma
// has a kernel in quot/aesw_quot.hip; the fold runs on the device cut into segments, aesw_vanish.h's.
// The field is aesw_fr.h's, omega, delta and the column order of the permutation aesw_sigma.h's, zeta aesw_ntt.h's, the arity of
// a tag aesw_theta.h's; nothing of them is restated.
// No HIP call and no ROCm include: the tests compile this header alone with g++.
//
// n = 2^k, E = 2^ext_k, m = E / n.  Row j of an extended column is the column's polynomial at x_j = zeta * omega_ext^j.  The
// numerator folds the constraints with  acc = acc * y + constraint  in this order (plonk/evaluation.rs of halo2_proofs v0.3.0
// restated from memory; parity with halo2's own order is not pinned by a test):
//   1. the gate              q_rcon * (words - rcon)
//   2. the permutation       l0 * (1 - Zp_0);  l_last * (Zp_(S-1)^2 - Zp_(S-1));  for s = 1 ... S-1: l0 * (Zp_s - Zp_(s-1)[rot U]);
//                            for s = 0 ... S-1: l_active * (Zp_s[rot 1] * prod_c (v_c + beta * sigma_c + gamma)
//                                                            - Zp_s * prod_c (v_c + beta * delta^c * x_j + gamma)),  c over set s
//   3. the lookups           for set s, tag t = 1 ... 5, q the selector of (s, t), a = theta_arity(theta_table_of_tag(t)),
//                            in = q * compress(t, x_s, y_s, z_s; a), tab = compress(the table columns; a):
//                            l0 * (1 - Z);  l_last * (Z^2 - Z);
//                            l_active * (Z[rot 1] * (A' + beta) * (S' + gamma) - Z * (in + beta) * (tab + gamma));
//                            l0 * (A' - S');  l_active * (A' - S') * (A' - A'[rot -1])
// and the output is acc * inv(x_j^n - 1).
#pragma once
#include <stdint.h>

#include "aesw_fr.h"
#include "aesw_ntt.h"
#include "aesw_sigma.h"
#include "aesw_theta.h"

#if defined(__HIPCC__)
#define AESW_QUOT_HD __host__ __device__ __forceinline__
#define AESW_QUOT_ROLLED _Pragma("unroll 1")  // a loop that stays a loop: its body is tens of field products of code
#else
#define AESW_QUOT_HD inline
#define AESW_QUOT_ROLLED
#endif

namespace aesw {

// ---- the shape and its bounds ---------------------------------------------------------------------------------------------------
struct QuotShape {
    uint32_t k, ext_k, zeta_sel, n_sets, chunk_len, n_rows;
};
constexpr uint32_t QUOT_MIN_K = NTT_MIN_K, QUOT_MAX_EXT_K = NTT_MAX_K, QUOT_MIN_LOG_M = 2, QUOT_MAX_SETS = MULT_MAX_SETS, QUOT_THREADS = 256;
AESW_QUOT_HD constexpr bool quot_k_ok(uint32_t k, uint32_t ext_k) { return k >= QUOT_MIN_K && ext_k <= QUOT_MAX_EXT_K && ext_k >= k && ext_k - k >= QUOT_MIN_LOG_M; }
AESW_QUOT_HD constexpr uint32_t quot_m(uint32_t k, uint32_t ext_k) { return 1u << (ext_k - k); }
AESW_QUOT_HD constexpr bool quot_sets_ok(uint32_t n_sets) { return n_sets >= 1 && n_sets <= QUOT_MAX_SETS; }
// the permutation constraint of a set has degree chunk_len + 2, and the extended domain holds degree m + 1
AESW_QUOT_HD constexpr bool quot_chunk_len_ok(uint32_t k, uint32_t ext_k, uint32_t chunk_len) {
    return sigma_chunk_len_ok(chunk_len) && chunk_len + 2u <= quot_m(k, ext_k) + 1u;
}
AESW_QUOT_HD constexpr bool quot_rows_ok(uint32_t k, uint32_t n_rows) { return n_rows >= 1 && n_rows < (1u << k); }
AESW_QUOT_HD constexpr bool quot_shape_ok(const QuotShape &q) {
    return quot_k_ok(q.k, q.ext_k) && q.zeta_sel <= 1 && quot_sets_ok(q.n_sets) && quot_chunk_len_ok(q.k, q.ext_k, q.chunk_len) && quot_rows_ok(q.k, q.n_rows);
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------
// a rotation by r rows of the circuit (r may be negative) reads this row of an extended column: (j + r * m) mod E
AESW_QUOT_HD constexpr uint32_t quot_rot(uint32_t k, uint32_t ext_k, uint32_t j, int32_t r) {
    return (j + ((uint32_t)r << (ext_k - k))) & ((1u << ext_k) - 1u);  // E is a power of two below 2^32: the wrap of uint32_t is the wrap mod E
}
// x_j^n = zeta^n * (omega_ext^n)^j takes m values: the cell of the vanishing table row j multiplies by
AESW_QUOT_HD constexpr uint32_t quot_vanish_index(uint32_t k, uint32_t ext_k, uint32_t j) { return j & (quot_m(k, ext_k) - 1u); }

// ---- the column groups of an evaluate call, in the order of its arguments ---------------------------------------------------------
enum QuotGroup : uint32_t { QUOT_ADVICE, QUOT_RCON, QUOT_SELECTOR, QUOT_TABLE, QUOT_SIGMA, QUOT_ZPERM, QUOT_A, QUOT_S, QUOT_ZLOOKUP, QUOT_L, QUOT_GROUPS };
AESW_QUOT_HD constexpr uint32_t quot_perm_sets(uint32_t n_sets, uint32_t chunk_len) { return sigma_sets(sigma_columns(n_sets), chunk_len); }
AESW_QUOT_HD constexpr uint32_t quot_group_columns(uint32_t group, uint32_t n_sets, uint32_t chunk_len) {
    return group == QUOT_ADVICE ? 3u * n_sets + 1u : group == QUOT_RCON ? 2u : group == QUOT_TABLE ? 4u : group == QUOT_SIGMA ? sigma_columns(n_sets)
         : group == QUOT_ZPERM ? quot_perm_sets(n_sets, chunk_len) : group == QUOT_L ? 3u : THETA_TAGS * n_sets;
}
AESW_QUOT_HD constexpr uint32_t quot_columns(uint32_t n_sets, uint32_t chunk_len) {
    uint32_t sum = 0;
    for (uint32_t g = 0; g < QUOT_GROUPS; ++g) sum += quot_group_columns(g, n_sets, chunk_len);
    return sum;
}
static_assert(quot_columns(4, 3) == 121, "the cells a row reads at N = 4, its rotations apart");

// ---- the tables -------------------------------------------------------------------------------------------------------------------
// vanish: inv(x^n - 1) for the m values of x^n, cell i that of the rows j with j mod m == i; low: omega_ext^j, j < 2^min(ext_k, 14);
// high: zeta * omega_ext^(j * 2^14), j < 2^max(ext_k - 14, 0) (4.21's split), so that x_j is one product.  Free of the challenges.
struct QuotTables {
    uint32_t vanish_at, low_at, high_at, cells;  // in cells
};
AESW_QUOT_HD constexpr QuotTables quot_tables(uint32_t k, uint32_t ext_k) {
    QuotTables t{};
    t.vanish_at = 0;
    t.low_at = quot_m(k, ext_k);
    t.high_at = t.low_at + ntt_low_cells(ext_k);
    t.cells = t.high_at + ntt_high_cells(ext_k);
    return t;
}
AESW_QUOT_HD constexpr uint64_t quot_tables_bytes(uint32_t k, uint32_t ext_k) { return quot_k_ok(k, ext_k) ? (uint64_t)quot_tables(k, ext_k).cells * sizeof(Fr) : 0u; }
static_assert(quot_tables_bytes(20, 22) == ((4u + (1u << 14) + (1u << 8)) * 32u) && quot_tables_bytes(25, 28) <= (1u << 20) + 1024u, "about 1 MiB where m is small");
// zeta = zeta0^(zeta_sel + 1); zeta^n = zeta0^((zeta_sel + 1) * 2^k mod 3), and 2^k mod 3 is 1 for an even k and 2 for an odd one: never 1
AESW_QUOT_HD constexpr uint32_t quot_zeta_n_exponent(uint32_t k, uint32_t zeta_sel) { return (zeta_sel + 1u) * (k % 2u ? 2u : 1u) % 3u; }
static_assert(quot_zeta_n_exponent(10, 0) != 0 && quot_zeta_n_exponent(10, 1) != 0 && quot_zeta_n_exponent(11, 0) != 0 && quot_zeta_n_exponent(11, 1) != 0,
              "zeta^n is a cube root of 1 that is not 1, no power of two's root of 1 is its inverse: x^n - 1 is never 0");
// cell `at` of the tables, as a tables kernel computes it
AESW_QUOT_HD constexpr Fr quot_table_cell(uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint32_t at) {
    const QuotTables t = quot_tables(k, ext_k);
    if (at < t.low_at) return fr_inv(fr_sub(fr_mul(ntt_zeta0_power(quot_zeta_n_exponent(k, zeta_sel)), fr_pow_u32(sigma_omega(ext_k - k), at)), FR_ONE));
    if (at < t.high_at) return fr_pow_u32(sigma_omega(ext_k), at - t.low_at);
    return fr_mul(ntt_zeta0_power(zeta_sel + 1u), fr_pow_u32(sigma_omega(ext_k), (at - t.high_at) << NTT_SPLIT));  // < 2^ext_k: no exponent wraps
}
// x_j from the tables: load(at) is cell `at` of them
template <class Cell>
AESW_QUOT_HD Fr quot_point(uint32_t k, uint32_t ext_k, uint32_t j, Cell &&cell) {
    const QuotTables t = quot_tables(k, ext_k);
    return fr_mul(cell(t.low_at + ntt_low_index(j)), cell(t.high_at + ntt_high_index(j)));
}

// ---- sigma as cells ---------------------------------------------------------------------------------------------------------------
// the cell an entry of the mapping names: itself where the entry is out of range (the rule of aesw_sigma.h's library)
AESW_QUOT_HD constexpr uint32_t quot_sigma_image(uint32_t k, uint32_t n_cols, uint32_t c, uint32_t i, uint32_t entry) {
    return sigma_cell_in_range(k, n_cols, entry) ? entry : sigma_cell_index(k, c, i);
}
// its label delta^c' * omega^i' from the tables of aesw_sigma.h (low, high, delta): cell(at) is cell `at` of them
template <class Cell>
AESW_QUOT_HD Fr quot_sigma_label(uint32_t k, uint32_t image, Cell &&cell) {
    const uint32_t row = sigma_cell_row(k, image), low = sigma_low_cells(k), high = sigma_high_cells(k);
    return fr_mul(cell(low + high + sigma_cell_col(k, image)), fr_mul(cell(sigma_low_index(row)), cell(low + sigma_high_index(row))));
}

// ---- the fold -----------------------------------------------------------------------------------------------------------------------
// the field products quot_numerator, the point x_j and the division take per row (what a measurement of a kernel is priced by)
AESW_QUOT_HD constexpr uint32_t quot_products_per_row(uint32_t n_sets, uint32_t chunk_len) {
    const uint32_t cols = sigma_columns(n_sets), sets = sigma_sets(cols, chunk_len);
    uint32_t p = 1;                        // x_j
    p += 1;                                // the gate; it opens the fold
    p += 2 + 3 + 2 * (sets - 1);           // Zp_0 opens, Zp_(S-1) closes at 0 or 1, the sets chain
    p += 1 + 4 * cols + 2 * sets;          // beta * x_j; per column beta * sigma, two running products, the next delta power; per set l_active and the fold
    p += 2 + 3;                            // theta^2, theta^3; the table under each arity
    p += n_sets * (2 + THETA_TAGS * 17);   // x_s, y_s, z_s under each arity; per argument 2 + 3 + 7 + 2 + 3
    p += 1;                                // the division
    return p;
}
static_assert(quot_products_per_row(4, 3) == 436, "12 + 4 S + 4 C + 87 N");

// a small integer times a cell, by additions
AESW_QUOT_HD Fr quot_times_small(const Fr &a, uint32_t t) {
    Fr acc = a;
    for (uint32_t u = 1; u < t; ++u) acc = fr_add(acc, a);
    return acc;
}
AESW_QUOT_HD Fr quot_pick(uint32_t arity, const Fr &two, const Fr &three, const Fr &four) {
    Fr out = FR_ZERO;
    AESW_MONT_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) out.l[i] = arity == 2 ? two.l[i] : arity == 3 ? three.l[i] : four.l[i];
    return out;
}

// The numerator at row j.  x = x_j; load(group, column, row) is the cell of that extended column at that row.  Every cell and
// challenge canonical.
template <class Load>
AESW_QUOT_HD Fr quot_numerator(const QuotShape &q, uint32_t j, const Fr &x, const Fr &theta, const Fr &beta, const Fr &gamma, const Fr &y, Load &&load) {
    const uint32_t next = quot_rot(q.k, q.ext_k, j, 1), prev = quot_rot(q.k, q.ext_k, j, -1), far = quot_rot(q.k, q.ext_k, j, (int32_t)q.n_rows);
    const uint32_t cols = sigma_columns(q.n_sets), sets = sigma_sets(cols, q.chunk_len), words = 3u * q.n_sets;
    const Fr one = FR_ONE, delta = SIGMA_DELTA;
    const Fr l0 = load(QUOT_L, 0, j), l_last = load(QUOT_L, 1, j), l_active = load(QUOT_L, 2, j);

    // 1. the gate
    Fr acc = fr_mul(load(QUOT_RCON, 1, j), fr_sub(load(QUOT_ADVICE, words, j), load(QUOT_RCON, 0, j)));
    const auto fold = [&](const Fr &constraint) { acc = fr_add(fr_mul(acc, y), constraint); };

    // 2. the permutation
    fold(fr_mul(l0, fr_sub(one, load(QUOT_ZPERM, 0, j))));
    {
        const Fr z = load(QUOT_ZPERM, sets - 1, j);
        fold(fr_mul(l_last, fr_sub(fr_mul(z, z), z)));
    }
    AESW_QUOT_ROLLED
    for (uint32_t s = 1; s < sets; ++s) fold(fr_mul(l0, fr_sub(load(QUOT_ZPERM, s, j), load(QUOT_ZPERM, s - 1, far))));
    Fr bx = fr_mul(beta, x);  // beta * delta^c * x_j, column by column
    AESW_QUOT_ROLLED
    for (uint32_t s = 0; s < sets; ++s) {
        Fr left = load(QUOT_ZPERM, s, next), right = load(QUOT_ZPERM, s, j);
        AESW_QUOT_ROLLED
        for (uint32_t c = sigma_set_first(s, q.chunk_len); c < sigma_set_end(s, q.chunk_len, cols); ++c) {
            const uint32_t source = sigma_source_of_column(q.n_sets, c);  // an advice column, or behind them the fixed one
            const Fr vg = fr_add(source <= words ? load(QUOT_ADVICE, source, j) : load(QUOT_RCON, 0, j), gamma);
            left = fr_mul(left, fr_add(vg, fr_mul(beta, load(QUOT_SIGMA, c, j))));
            right = fr_mul(right, fr_add(vg, bx));
            bx = fr_mul(bx, delta);
        }
        fold(fr_mul(l_active, fr_sub(left, right)));
    }

    // 3. the lookups: the table under each arity once per row, x_s, y_s, z_s under each arity once per set, q factored out of `in`
    const Fr theta2 = fr_mul(theta, theta), theta3 = fr_mul(theta2, theta);
    const Fr tab2 = fr_add(fr_mul(load(QUOT_TABLE, 0, j), theta), load(QUOT_TABLE, 1, j));
    const Fr tab3 = fr_add(fr_mul(tab2, theta), load(QUOT_TABLE, 2, j));
    const Fr tab4 = fr_add(fr_mul(tab3, theta), load(QUOT_TABLE, 3, j));
    AESW_QUOT_ROLLED
    for (uint32_t s = 0; s < q.n_sets; ++s) {
        const Fr in2 = load(QUOT_ADVICE, 3u * s, j);
        const Fr in3 = fr_add(fr_mul(in2, theta), load(QUOT_ADVICE, 3u * s + 1u, j));
        const Fr in4 = fr_add(fr_mul(in3, theta), load(QUOT_ADVICE, 3u * s + 2u, j));
        AESW_QUOT_ROLLED
        for (uint32_t t = 1; t <= THETA_TAGS; ++t) {
            const uint32_t arity = theta_arity(theta_table_of_tag(t)), at = s * THETA_TAGS + t - 1u;
            // compress(t, x, y, z) = t * theta^(arity - 1) + (x, y, z under the arity)
            const Fr in = fr_mul(load(QUOT_SELECTOR, at, j), fr_add(quot_times_small(quot_pick(arity, theta, theta2, theta3), t), quot_pick(arity, in2, in3, in4)));
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
    }
    return acc;
}

}  // namespace aesw
