/* aesw_theta.h -- C ABI of libaesw_theta.so: the lookup arguments compressed under theta, on the device.
 *
 * halo2's lookup argument compresses the expressions of an input row and of a table row into one Fr cell each,
 * acc = acc * theta + e over the expressions in order, and commits to four columns per argument: the compressed inputs and the
 * compressed table in row order, and their permuted forms A' and S'.  The permuted-columns library arranges A' and S' as
 * columns of table-ROW INDICES without theta.  This library adds what is left once theta is known:
 *   1. the three compressed tables -- the five arguments have three arities -- from theta and the context's runtime tables;
 *   2. the compressed INPUT column in row order, again as table-row indices, from the witness slabs where they lie;
 *   3. one gather that turns an index column of all 5 * n_sets arguments into Fr cells, every argument through the table of
 *      its own arity.
 * Four calls of (3) -- with the indices of (2), with NULL for the table column in row order, with d_a and with d_s of the
 * permuted-columns library -- give the four columns commit_permuted commits to; the host uploads the 32 bytes of theta.
 *
 * AN Fr CELL is 32 bytes: eight little-endian 32-bit limbs of v * 2^256 mod r, r the order of bn256's scalar field -- the
 * Montgomery form halo2curves keeps in memory and every Fr cell of aesw.h.
 *
 * THE ARGUMENT (set s, tag t), t = 1 U8, 2 Xor, 3 Sbox, 4 GfMul2, 5 GfMul3, lies at ((s * 5 + t - 1) << k) of every column
 * of this header, as in the permuted-columns library.  Its table is j(t): j(1) = 0, j(3) = j(4) = j(5) = 1, j(2) = 2.
 *
 * Every device call is asynchronous on `stream`, waits for nothing on the host, writes every output byte itself with plain
 * stores -- no atomic, nothing to reset -- and may be captured into a hipGraph: a replay rebuilds its outputs and its report.
 * A refusal returns AESW_ERR_INVALID_ARG (or AESW_ERR_CAPACITY) with nothing enqueued and the outputs untouched;
 * aesw_last_error names the call.  A group context is refused.
 *
 * This header includes aesw_mult.h for AESW_TABLE_ROWS, aesw_mult_report and the bin rule only: the library links against
 * libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_theta -laesw. */
#ifndef AESW_THETA_H
#define AESW_THETA_H

#include <stddef.h>

#include "aesw_mult.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_THETA_TABLES 3u    /* arities 2, 3 and 4 */
#define AESW_THETA_ARGUMENTS 5u /* per set: tags 1 ... 5 */
#define AESW_THETA_MISS 0xffffffffu /* the input index of an enabled lookup that names no table row */

typedef struct aesw_theta_report {
    uint64_t cells;        /* cells written: 3 * AESW_TABLE_ROWS */
    uint64_t noncanonical; /* 1: theta >= r, every cell is zero */
} aesw_theta_report;

/* The three compressed tables.  d_theta: one Fr cell in device memory, 16-byte aligned, read when the kernel runs (a replay
 * follows what it then holds).  d_table_fr: [3][AESW_TABLE_ROWS][32] bytes, 16-byte aligned.  Table j compresses row
 * (tag, a, b, c) of aesw_lookup_table -- built from the context's runtime tables -- over its first j + 2 expressions:
 *   j = 0  tag * theta + a        j = 1  (tag * theta + a) * theta + b        j = 2  ((tag * theta + a) * theta + b) * theta + c
 * Every table holds all 66 561 rows (an argument reads the rows of its own section and row 66 560 only); row 66 560 is 32 zero
 * bytes in all three.  A theta that is not canonical has no defined result: every cell is written as zero and
 * d_report->noncanonical is 1.  d_report: 8-byte aligned, set by the call. */
int aesw_theta_compress_table_device(aesw_ctx *ctx, const uint8_t *d_theta, uint8_t *d_table_fr,
                                     aesw_theta_report *d_report, void *stream);

/* The compressed inputs of ONE FixedAes128Config<k, n_sets> circuit in row order, as table-row indices.  The circuit's first
 * n_blocks blocks (slabs d_x, d_y, d_z of `layout`: DENSE or PACKED; VALUES has no x: AESW_ERR_INVALID_ARG) sit where
 * aesw_block_placement puts them, its key slab (NULL, or with kx, ky or kz NULL: no key lookups; w is not read) at the key
 * rows of set 0.  d_in: [n_sets][5][2^k] uint32_t, 16-byte aligned; cell (s, t, i) is
 *   aesw_mult_bin(t, x, y)   where row i of set s holds an enabled lookup of tag t that is a hit,
 *   AESW_THETA_MISS          where it holds an enabled lookup of tag t that is a miss,
 *   AESW_TABLE_ROWS - 1      (the all-zero row) everywhere else: rows of other tags, copy rows, rows no block fills, and for
 *                            k < 9 -- 2^k rows do not hold the key rows -- every row of set 0.
 * All 2^k rows of every argument are written, each word once; blinding rows are the caller's to overwrite.  d_report
 * (8-byte aligned) is set by the call: lookups, misses and first_miss as aesw_mult_count_device reports them over the same
 * slabs as one circuit (unit: the circuit's block index, 0 for the key slab).
 * k 2 ... 30, n_sets 1 ... 1024, n_blocks <= aesw_block_capacity(k, n_sets), else AESW_ERR_CAPACITY.  The slabs and key columns
 * are 16-byte aligned (d_x, d_y, d_z may be NULL when n_blocks is 0).
 *
 * The call reduces the report through a workspace the library keeps per (context, stream): 16 bytes per 1 024 rows of a set
 * (16 GiB at k = 30 with 1 024 sets, where one workgroup folds 2^30 parts: such a circuit is accepted, not fast).  A call makes
 * or enlarges the workspace of its context and stream itself -- the only time it allocates -- except while `stream` is
 * capturing, where it refuses and names aesw_theta_prepare: prepare the shape for the capturing stream first.  A workspace that
 * was handed out is never freed or moved while the process lives (a larger shape gets a new block next to it), so a captured
 * call stays valid whatever is prepared or called afterwards.  A graph captured on a stream uses that stream's workspace when
 * it is replayed, on whichever stream: do not run a replay and another inputs call of the same context and capture stream
 * at once.  Calls on different contexts or different streams share nothing. */
int aesw_theta_inputs_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout,
                             const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slab,
                             uint32_t *d_in, aesw_mult_report *d_report, void *stream);

/* Makes the workspace aesw_theta_inputs_device uses for this context on `stream` hold a circuit of (k, n_sets), and anything
 * smaller.  Allocates when it has to grow, and frees nothing. */
int aesw_theta_prepare(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, void *stream);

/* All 5 * n_sets arguments of an index column as Fr cells: for every argument (s, t) and i < n_rows
 *   d_out_fr[((s * 5 + t - 1) << k) + i] = d_table_fr[j(t)][d_index[((s * 5 + t - 1) << k) + i]]
 * 32 bytes each.  Rows n_rows ... 2^k - 1 are not written.  An index >= AESW_TABLE_ROWS (AESW_THETA_MISS included) gives a cell
 * of 32 zero bytes and reads nothing.  d_index == NULL: the compressed TABLE column in row order -- index i for
 * i < AESW_TABLE_ROWS, pad_row behind it (the row the circuit's table columns hold below the table; not read otherwise, but
 * checked).  d_index [n_sets][5][2^k] uint32_t, 4-byte aligned; d_table_fr as aesw_theta_compress_table_device leaves it and
 * d_out_fr [n_sets][5][2^k][32] 16-byte aligned.  k 17 ... 30, n_sets 1 ... 1024, AESW_TABLE_ROWS <= n_rows <= 2^k,
 * pad_row < AESW_TABLE_ROWS.  The stores follow the context's "fr_store_mode", as aesw_expand_fr_device's. */
int aesw_theta_columns_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row,
                              const uint32_t *d_index, const uint8_t *d_table_fr, uint8_t *d_out_fr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_THETA_H */
