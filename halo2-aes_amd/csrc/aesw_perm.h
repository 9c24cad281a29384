// aesw_perm.h -- the arrangement rule of plookup's permuted columns, once: which table row stands at every position of the
// permuted input column A' and of the permuted table column S' of ONE lookup argument, given the histogram of the argument's
// set.  One source for the kernels of libaesw_perm.so, a sequential statement of the same rule
// (perm_scan_host, perm_cell) and the CPU test that holds it against tests/perm_model.py.  The sections of the table and the
// bins are aesw_mult.h's: nothing of them is restated here.
// No HIP call and no ROCm include: tests/test_perm_model.py compiles this header alone with g++.
//
// The argument (set s, tag t in 1 ... 5) runs over u rows, MULT_BINS <= u <= 2^k; H is the set's histogram.
//   counts   c[r] = H[r] inside the section of t, consumed in ascending row order until u is reached: with `before` the sum of
//            the section's bins below r,  c[r] = clamp(u - before, 0, H[r]).  c[r] = 0 for every other row below MULT_ZERO_ROW --
//            the bins of other sections are never read --, and c[MULT_ZERO_ROW] = u - sum(c): the rows whose selector is off.
//   A'       the rows in ascending order, row r c[r] times: A'[i] = r for P[r] <= i < P[r] + c[r], P the exclusive prefix of c.
//   S'       at the first position of every non-empty run the run's row; the other u - D positions (D = rows with c > 0), in
//            ascending order, take the leftover list: the rows with c == 0 in ascending order, then u - MULT_BINS copies of
//            pad_row -- the table row the circuit's table columns hold below row MULT_ZERO_ROW.
// Then A' is a permutation of the argument's inputs, S' one of the table column over u rows, A'[0] == S'[0], and A'[i] == S'[i]
// or A'[i] == A'[i - 1] everywhere else.
//
// Every count is clipped to u + 1 before it is added and every sum again (perm_sat_add): the clipped sum of non-negative
// numbers is associative, needs 32 bits for u <= 2^30 whatever the bins hold, and "the section sums to more than u" is "the
// clipped sum is u + 1".  The start of row r's run is min(clipped sum of the bins below r, u).
#pragma once
#include "aesw_mult.h"

namespace aesw {

constexpr uint32_t PERM_MIN_K = 17, PERM_TAGS = 5;
static_assert((1u << PERM_MIN_K) >= MULT_BINS && (1u << (PERM_MIN_K - 1)) < MULT_BINS, "the smallest circuit that holds the table");
AESW_HD constexpr bool perm_k_ok(uint32_t k) { return k >= PERM_MIN_K && k <= MULT_MAX_K; }
AESW_HD constexpr bool perm_rows_ok(uint32_t k, uint32_t u) { return u >= MULT_BINS && u <= (1u << k); }

AESW_HD constexpr uint32_t perm_clip(uint32_t v, uint32_t u) { return v < u + 1 ? v : u + 1; }
// a, b <= u + 1 <= 2^30 + 1: the sum fits
AESW_HD constexpr uint32_t perm_sat_add(uint32_t a, uint32_t b, uint32_t u) { return perm_clip(a + b, u); }
AESW_HD constexpr uint32_t perm_start(uint32_t clipped_before, uint32_t u) { return clipped_before < u ? clipped_before : u; }

// The workspace: per set PERM_WS_WORDS uint32_t.  An argument has three arrays of as many words as its section has rows -- the
// start P of every row's run, the INCLUSIVE count of the rows with c > 0 up to every row, the section's rows with c == 0 in
// ascending order -- in the order of the tags, and behind the arrays of all five its four scalars (PermScalars).
struct PermScalars {
    uint32_t z;         // the section's clamped sum: where the all-zero run starts (u: there is none)
    uint32_t d;         // rows of the section with c > 0
    uint32_t zero_used; // z < u
    uint32_t overflow;  // the section summed to more than u: the counts were clamped
};
AESW_HD constexpr uint32_t perm_ws_arrays(uint32_t tag) {
    uint32_t w = 0;
    for (uint32_t t = 1; t < tag; ++t) w += 3 * mult_section_rows(t);
    return w;
}
constexpr uint32_t PERM_WS_SCALARS = perm_ws_arrays(PERM_TAGS + 1), PERM_WS_WORDS = PERM_WS_SCALARS + 32;
static_assert(PERM_WS_SCALARS == 3 * (MULT_BINS - 1) && PERM_WS_SCALARS % 4 == 0 && PERM_WS_WORDS % 4 == 0 && PERM_TAGS * 4 <= 32,
              "every array and the scalars start 16-byte aligned");
AESW_HD constexpr uint32_t perm_ws_scalars(uint32_t tag) { return PERM_WS_SCALARS + 4 * (tag - 1); }

// What a position needs to know of its argument.
struct PermArgument {
    uint32_t first, rows;      // the section (aesw_mult.h)
    uint32_t u, pad_row;
    PermScalars sc;
    const uint32_t *start, *used, *unused;  // the three arrays
};
AESW_HD constexpr PermArgument perm_argument(const uint32_t *ws_of_set, uint32_t tag, uint32_t u, uint32_t pad_row) {
    const uint32_t rows = mult_section_rows(tag);
    const uint32_t *a = ws_of_set + perm_ws_arrays(tag), *s = ws_of_set + perm_ws_scalars(tag);
    return PermArgument{mult_section_first(tag), rows, u, pad_row, PermScalars{s[0], s[1], s[2], s[3]}, a, a + rows, a + 2 * rows};
}

// The largest j in [lo, hi) with start[j] <= i, given start[lo] <= i; `at` comes in as start[lo] and goes out as start[j].
// start does not decrease and a row with c == 0 starts where the next one does, so for i < z row j has c > 0: it is A'[i].
AESW_HD constexpr uint32_t perm_search(const uint32_t *start, uint32_t i, uint32_t lo, uint32_t hi, uint32_t &at) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2, v = start[mid];
        if (v <= i) { lo = mid; at = v; }
        else hi = mid;
    }
    return lo;
}

// Entry q of the leftover list: the rows with c == 0 in ascending order -- every row in front of the section, the section's
// unused rows, every row behind the section, the all-zero row if no selector is off -- then pad_row.
AESW_HD constexpr uint32_t perm_leftover(const PermArgument &a, uint32_t q) {
    if (q < a.first) return q;
    q -= a.first;
    const uint32_t n_unused = a.rows - a.sc.d;
    if (q < n_unused) return a.unused[q];
    q -= n_unused;
    const uint32_t behind = MULT_ZERO_ROW - (a.first + a.rows);
    if (q < behind) return a.first + a.rows + q;
    q -= behind;
    return q == 0 && !a.sc.zero_used ? MULT_ZERO_ROW : a.pad_row;
}

// S'[i], given A'[i] = first + j with the run starting at `at` (i < z), or the all-zero row (i >= z, j ignored): the run's row at
// its first position; elsewhere the leftover entry whose index is i minus the runs that have started at or before i.
AESW_HD constexpr uint32_t perm_table_cell(const PermArgument &a, uint32_t i, uint32_t j, uint32_t at) {
    if (i < a.sc.z) return i == at ? a.first + j : perm_leftover(a, i - a.used[j]);
    return i == a.sc.z ? MULT_ZERO_ROW : perm_leftover(a, i - a.sc.d - 1);
}

struct PermCell {
    uint32_t a, s;
};
// Position i < u on its own (the kernel shares the search among a lane's four positions).
AESW_HD constexpr PermCell perm_cell(const PermArgument &a, uint32_t i) {
    if (i >= a.sc.z) return PermCell{MULT_ZERO_ROW, perm_table_cell(a, i, 0, 0)};
    uint32_t at = 0;
    const uint32_t j = perm_search(a.start, i, 0, a.rows, at);
    return PermCell{a.first + j, perm_table_cell(a, i, j, at)};
}

// The scan of one argument, row after row: what perm_scan_kernel computes tile by tile.  `hist` is the set's histogram, `ws` the
// set's workspace.
inline void perm_scan_host(const uint32_t *hist, uint32_t tag, uint32_t u, uint32_t *ws) {
    const uint32_t first = mult_section_first(tag), rows = mult_section_rows(tag);
    uint32_t *start = ws + perm_ws_arrays(tag), *used = start + rows, *unused = used + rows, *sc = ws + perm_ws_scalars(tag);
    uint32_t before = 0, d = 0;
    for (uint32_t j = 0; j < rows; ++j) {
        const uint32_t next = perm_sat_add(before, perm_clip(hist[first + j], u), u);
        start[j] = perm_start(before, u);
        if (perm_start(next, u) > start[j]) ++d;
        else unused[j - d] = first + j;
        used[j] = d;
        before = next;
    }
    sc[0] = perm_start(before, u); sc[1] = d; sc[2] = sc[0] < u; sc[3] = before > u;
}

}  // namespace aesw
