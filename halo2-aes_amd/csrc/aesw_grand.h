// aesw_grand.h -- the rules of libaesw_grand.so, once: what an index of a column reads, what a row of an
// argument contributes to halo2's lookup grand product, how a lane inverts a batch of table cells with one inversion, and how
// the rows of an argument are cut into the chunks the three passes of grand/aesw_grand.hip share.  One source for the kernels
// and for the CPU test of the rules.  Nothing is restated: the field is aesw_fr.h's, the table of a tag and the row-order table
// index aesw_theta.h's, the bounds aesw_mult.h's.
// No HIP call and no ROCm include: tests/test_grand_model.py compiles this header alone with g++.
#pragma once
#include "aesw_theta.h"

namespace aesw {

#ifndef AESW_GRAND_BATCH
#define AESW_GRAND_BATCH 8  // table cells a lane inverts with one fr_inv (4.20, "Measured": the values tried)
#endif
#ifndef AESW_GRAND_ROWS_PER_LANE
#define AESW_GRAND_ROWS_PER_LANE 4  // consecutive rows of Z a lane of the chunk and scan kernels owns
#endif
constexpr uint32_t GRAND_BATCH = AESW_GRAND_BATCH, GRAND_ROWS_PER_LANE = AESW_GRAND_ROWS_PER_LANE;
constexpr uint32_t GRAND_THREADS = 256, GRAND_CHUNK = GRAND_THREADS * GRAND_ROWS_PER_LANE;  // rows of one workgroup
constexpr uint32_t GRAND_PLANES = 2;  // of the inverse table: 1 / (T + beta), 1 / (T + gamma)
static_assert(GRAND_BATCH >= 1 && GRAND_BATCH <= 16, "a lane keeps the batch's running products in registers");
static_assert(GRAND_ROWS_PER_LANE == 2 || GRAND_ROWS_PER_LANE == 4, "a lane reads its rows of an index column with one load of 8 or 16 bytes");

AESW_HD constexpr bool grand_k_ok(uint32_t k) { return k >= 17 && k <= MULT_MAX_K; }  // 2^k rows hold the table

// The table row an index of a column reads: itself below the table's end, the all-zero row for anything larger (THETA_MISS
// among them) -- row 66 560 compresses to the zero cell in all three tables, which is the cell the columns call writes there.
AESW_HD constexpr uint32_t grand_row_of_index(uint32_t x) { return x < MULT_BINS ? x : MULT_ZERO_ROW; }

// Montgomery's trick over B sums sum(0) ... sum(B - 1) (a callable: the sums are made twice, never kept): one fr_inv of the
// product of the sums that are not zero, out(i, inverse) for every i -- the zero cell for a zero sum, which the running product
// skips.  Returns how many sums were zero.  B products forwards, 2 B backwards, one inversion.
template <int B, class Sum, class Out>
AESW_MONT_HD uint32_t grand_batch_invert(Sum &&sum, Out &&out) {
    Fr before[B];  // before[i]: the product of the non-zero sums below i
    Fr acc = FR_ONE;
    fr_unrolled<B>([&](auto at) {
        constexpr int i = decltype(at)::value;
        before[i] = acc;
        const Fr s = sum(i);
        if (!fr_is_zero(s)) acc = fr_mul(acc, s);
    });
    Fr inv = fr_inv(acc);  // acc is a product of non-zero values: never 0
    uint32_t zeros = 0;
    fr_unrolled<B>([&](auto at) {
        constexpr int i = B - 1 - decltype(at)::value;
        const Fr s = sum(i);
        if (fr_is_zero(s)) {
            out(i, FR_ZERO);
            ++zeros;
        } else {
            out(i, fr_mul(inv, before[i]));
            inv = fr_mul(inv, s);
        }
    });
    return zeros;
}

// What row i of an argument multiplies Z by: t_in, t_tab the table's cells at the input index and at theta_table_index(i, pad_row),
// inv_a = inv(T[a[i]] + beta) and inv_s = inv(T[s[i]] + gamma) out of the inverse table.  Three products.
AESW_MONT_HD constexpr Fr grand_row(const Fr &t_in, const Fr &t_tab, const Fr &inv_a, const Fr &inv_s, const Fr &beta, const Fr &gamma) {
    return fr_mul(fr_mul(fr_add(t_in, beta), fr_add(t_tab, gamma)), fr_mul(inv_a, inv_s));
}

// The rows of an argument: rows 0 ... grand_last_row are written (row n_rows holds the closing product where 2^k has room for
// it), in chunks of GRAND_CHUNK rows; the factors are those of the rows below n_rows.
AESW_HD constexpr uint32_t grand_last_row(uint32_t k, uint32_t n_rows) { return n_rows < (1u << k) ? n_rows : (1u << k) - 1; }
AESW_HD constexpr uint32_t grand_chunks(uint32_t k, uint32_t n_rows) { return grand_last_row(k, n_rows) / GRAND_CHUNK + 1; }
AESW_HD constexpr uint32_t grand_chunk_stride(uint32_t k) { return (1u << k) / GRAND_CHUNK; }  // chunks of 2^k rows: what an argument has room for
static_assert(grand_chunks(17, 1u << 17) == grand_chunk_stride(17) && grand_chunks(30, (1u << 30) - 1) == grand_chunk_stride(30) && grand_chunks(17, GRAND_CHUNK) == 2,
              "no n_rows needs more chunks than the stride");

// The workspace: one cell per chunk of every argument, then one 16-byte part of the report per argument.
AESW_HD constexpr uint64_t grand_workspace_cells(uint32_t k, uint32_t n_sets) { return (uint64_t)n_sets * THETA_TAGS * grand_chunk_stride(k); }
AESW_HD constexpr uint64_t grand_workspace_bytes(uint32_t k, uint32_t n_sets) {
    return grand_k_ok(k) && mult_sets_ok(n_sets) ? grand_workspace_cells(k, n_sets) * sizeof(Fr) + (uint64_t)n_sets * THETA_TAGS * 16u : 0u;
}

// The key of an open argument in the report: the encoding of aesw_perm_report.first_overflow.
AESW_HD constexpr uint64_t grand_argument_key(uint32_t argument) { return (uint64_t)(argument / THETA_TAGS) * 8u + argument % THETA_TAGS + 1u; }

}  // namespace aesw
