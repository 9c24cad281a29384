/* aesw_grand.h -- C ABI of libaesw_grand.so: the grand product Z of every lookup argument, on the device, from beta and gamma.
 *
 * halo2's lookup argument (halo2_proofs' commit_product) commits, after the challenges beta and gamma, to one column Z per
 * argument: with A the compressed inputs and S the compressed table in row order and A', S' their permuted forms,
 *   Z[0] = 1,   Z[i + 1] = Z[i] * (A[i] + beta) * (S[i] + gamma) / ((A'[i] + beta) * (S'[i] + gamma))   for i < n_rows,
 * and Z[n_rows] -- the closing product -- is 1 exactly when A', S' permute A, S over the usable rows.  The libraries of the
 * permuted columns and of the compression under theta leave all four columns as columns of table-ROW INDICES next to the three
 * compressed tables, so every value in them is one of 3 * 66 561 cells: this library inverts those cells once per proof
 * (2 * 3 * 66 561 inversions, batched, instead of 2^k per argument) and then builds Z of all 5 * n_sets arguments from the
 * index columns alone -- four gathers, three field products and a prefix product per row.
 *
 * AN Fr CELL is 32 bytes: eight little-endian 32-bit limbs of v * 2^256 mod r, r the order of bn256's scalar field -- the
 * Montgomery form halo2curves keeps in memory and every Fr cell of aesw.h.
 *
 * THE ARGUMENT (set s, tag t), t = 1 U8, 2 Xor, 3 Sbox, 4 GfMul2, 5 GfMul3, lies at ((s * 5 + t - 1) << k) of every column
 * of this header.  Its table is j(t): j(1) = 0, j(3) = j(4) = j(5) = 1, j(2) = 2 -- the table choice of the theta library.
 * THE VALUE AT AN INDEX x of a column of argument (s, t) is T_j(t)[x] for x < AESW_TABLE_ROWS and the zero cell for any larger
 * index (the miss marker 0xffffffff of the input column among them): the rule of the theta library's columns call.
 *
 * inv(0) = 0, the convention of ff's batch_invert, which halo2 uses: a zero term makes Z zero from its row on, and is reported.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, writes every output word
 * itself with plain stores -- no atomic, nothing to reset -- and may be captured into a hipGraph: a replay rebuilds its outputs
 * and its report from what beta, gamma and the columns then hold.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued
 * and the outputs untouched; aesw_last_error names the call.  A group context is refused.
 *
 * This header includes aesw_mult.h for AESW_TABLE_ROWS only: the library links against libaesw.so alone ($ORIGIN) and takes the
 * aesw_ctx that aesw_create made.  Link with -laesw_grand -laesw. */
#ifndef AESW_GRAND_H
#define AESW_GRAND_H

#include <stddef.h>

#include "aesw_mult.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_GRAND_PLANES 2u /* of the inverse table: 1 / (T + beta), 1 / (T + gamma) */

typedef struct aesw_grand_invert_report {
    uint64_t cells;        /* cells written: 2 * 3 * AESW_TABLE_ROWS */
    uint64_t noncanonical; /* 1: beta >= r or gamma >= r, every cell is zero */
    uint64_t zero_terms;   /* cells whose sum T + beta or T + gamma was zero: their inverse is the zero cell */
} aesw_grand_invert_report;

typedef struct aesw_grand_report {
    uint64_t arguments;  /* arguments built by this call: 5 * n_sets */
    uint64_t open;       /* arguments whose closing product is not 1 */
    uint64_t first_open; /* AESW_CHECK_NONE, or the smallest set * 8 + tag among them */
} aesw_grand_report;

/* The inverse table.  d_table_fr: [3][AESW_TABLE_ROWS][32] bytes, the three compressed tables as the theta library's table
 * call leaves them.  d_beta, d_gamma: one Fr cell each in device memory, 16-byte aligned, read when the kernel runs (a replay
 * follows what they then hold).  d_inv_fr: [2][3][AESW_TABLE_ROWS][32] bytes (12 779 712), 16-byte aligned:
 *   plane 0  inv(T_j[r] + beta)        plane 1  inv(T_j[r] + gamma)
 * A beta or gamma that is not canonical has no defined result: every cell is written as zero and d_report->noncanonical is 1
 * (zero_terms is then 0).  d_report: 8-byte aligned, set by the call. */
int aesw_grand_invert_table_device(aesw_ctx *ctx, const uint8_t *d_table_fr, const uint8_t *d_beta, const uint8_t *d_gamma,
                                   uint8_t *d_inv_fr, aesw_grand_invert_report *d_report, void *stream);

/* Pure host: the bytes of d_workspace for a circuit of (k, n_sets) -- a multiple of 16; 0 for k outside 17 ... 30 or n_sets
 * outside 1 ... 1024.  32 bytes per 1 024 rows of an argument and 16 bytes per argument.  Its content between calls is of no
 * interest; two calls in flight at once need two workspaces. */
size_t aesw_grand_workspace_bytes(uint32_t k, uint32_t n_sets);

/* Z of the 5 * n_sets arguments of one FixedAes128Config<k, n_sets> circuit: for every argument (s, t) and i < n_rows
 *   f[i] = (T_j[d_in[i]] + beta) * (T_j[tidx(i)] + gamma) * d_inv_fr[0][j][d_a[i]] * d_inv_fr[1][j][d_s[i]]
 *   Z[0] = 1,   Z[i + 1] = Z[i] * f[i]
 * with j = j(t), every index read by the rule above, and tidx(i) = i for i < AESW_TABLE_ROWS, pad_row behind it.
 *   d_in            the input column in row order, as the theta library's inputs call writes it
 *   d_a / d_s       the permuted columns A' and S', as the permuted-columns library's build call writes them
 *                   all three [n_sets][5][2^k] uint32_t, 16-byte aligned; rows 0 ... n_rows - 1 are used -- they are read four
 *                   at a time, so up to three rows behind n_rows (inside the 2^k) are read and their values ignored
 *   d_table_fr      [3][AESW_TABLE_ROWS][32], d_inv_fr [2][3][AESW_TABLE_ROWS][32] of the call above, 16-byte aligned.  A beta
 *                   or gamma that is not canonical is not this call's to detect: it trusts d_inv_fr and reads d_beta and
 *                   d_gamma (one cell each, 16-byte aligned) for the numerators only
 *   d_z_fr          [n_sets][5][2^k][32], 16-byte aligned: rows 0 ... min(n_rows, 2^k - 1) of every argument are written, each
 *                   word once -- row n_rows holds the closing product where 2^k has a row for it; the rows above it are the
 *                   caller's blinding rows and are not written
 *   d_closing_fr    [n_sets][5][32], 16-byte aligned: Z[n_rows] of every argument, always written
 *   d_workspace     aesw_grand_workspace_bytes(k, n_sets) bytes, 16-byte aligned
 *   d_report        8-byte aligned; set by the call
 * k 17 ... 30 (2^k rows hold the table), n_sets 1 ... 1024, AESW_TABLE_ROWS <= n_rows <= 2^k, pad_row < AESW_TABLE_ROWS.
 * The stores of Z follow the context's "fr_store_mode", as aesw_expand_fr_device's. */
int aesw_grand_product_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row,
                              const uint32_t *d_in, const uint32_t *d_a, const uint32_t *d_s,
                              const uint8_t *d_table_fr, const uint8_t *d_inv_fr, const uint8_t *d_beta, const uint8_t *d_gamma,
                              uint8_t *d_z_fr, uint8_t *d_closing_fr, void *d_workspace, aesw_grand_report *d_report,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_GRAND_H */
