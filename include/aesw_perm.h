/* aesw_perm.h -- C ABI of libaesw_perm.so: plookup's permuted columns, arranged on the device from the lookup multiplicities.
 *
 * A plookup prover (halo2_proofs' permute_expression_pair) sorts, for every lookup argument, the 2^k compressed inputs and
 * rearranges the table against them.  The histograms of aesw_mult.h / aesw_acc.h say the same thing without a sort: how often
 * every table row is an input.  This library turns the histogram of a set into the ARRANGEMENT of the set's five arguments:
 * for every position of the permuted input column A' and of the permuted table column S' the table ROW that stands there, as
 * an index into the 66 561 rows of aesw_lookup_table.  That needs no challenge.  Once theta is known the host compresses the
 * table once (66 561 cells, whatever the argument's arity) and aesw_perm_gather_fr_device turns every index into its cell.
 *
 * THE ARGUMENT (set s, tag t) -- t = 1 U8, 2 Xor, 3 Sbox, 4 GfMul2, 5 GfMul3, the tag column of the table -- runs over
 * n_rows = u rows, the host's usable rows (AESW_TABLE_ROWS <= u <= 2^k); rows u ... 2^k - 1 of both outputs are the host's
 * blinding rows and are NOT WRITTEN.  With H = d_mult[s] and the section of t the bin range of aesw_mult_bin:
 *   counts  c[r] = H[r] inside the section, 0 in every other row below 66 560 (the bins of other sections are never read, garbage
 *           there does not matter); if the section sums to more than u -- no histogram of a circuit of u rows does -- the counts
 *           are consumed in ascending row order until u is reached and the rest is dropped; c[66 560] = u - sum(c), the rows
 *           where the argument's selector is off: their input is the all-zero row.
 *   A'      the rows in ascending order, row r c[r] times: the all-zero run comes last.
 *   S'      at the first position of every non-empty run the run's row; the remaining positions, in ascending order, take the
 *           rows with c[r] == 0 in ascending order and then u - 66 561 copies of pad_row.
 * So A' is a permutation of the argument's inputs, S' one of the table column over u rows, A'[0] == S'[0], and A'[i] == S'[i]
 * or A'[i] == A'[i - 1] for every i > 0: plookup's relations, for every histogram.
 *
 * pad_row is the table row the circuit's table columns hold below row 66 560.  halo2's table layouter is believed to fill the
 * unassigned rows of a table column with the value assigned at offset 0 -- for src/table.rs row 0, (U8, 0, 0, 0) -- but that is
 * upstream's to say, so the caller decides: pass 0 for that, 66 560 for a zero-filled table.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host and may be captured into a
 * hipGraph; a replay rebuilds the columns and the report, it does not accumulate.  A refusal returns AESW_ERR_INVALID_ARG with
 * nothing enqueued and the outputs untouched; aesw_last_error names the call.  A group context is refused.
 *
 * This header includes aesw_mult.h for AESW_TABLE_ROWS and the bin layout only: the library links against libaesw.so alone
 * ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_perm -laesw. */
#ifndef AESW_PERM_H
#define AESW_PERM_H

#include <stddef.h>

#include "aesw_mult.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_PERM_ARGUMENTS 5u /* per set: tags 1 ... 5 */

typedef struct aesw_perm_report {
    uint64_t arguments;      /* arguments built by this call: 5 * n_sets */
    uint64_t overflowed;     /* arguments whose section summed to more than n_rows (their counts were clamped) */
    uint64_t first_overflow; /* AESW_CHECK_NONE, or the smallest set * 8 + tag among them */
} aesw_perm_report;

/* Pure host: the bytes of d_workspace for n_sets sets (0 for n_sets outside 1 ... 1024).  Its content between calls is of no
 * interest; two calls in flight at once need two workspaces. */
size_t aesw_perm_workspace_bytes(uint32_t n_sets);

/* Arranges the 5 * n_sets arguments of one FixedAes128Config<k, n_sets> circuit.
 *   d_mult       [n_sets][AESW_TABLE_ROWS] uint32_t, as any of the multiplicity libraries leaves it, 16-byte aligned
 *   d_a / d_s    each [n_sets][5][2^k] uint32_t, 16-byte aligned: argument (s, t) at ((s * 5 + t - 1) << k); rows 0 ... n_rows - 1
 *                of every argument are written, each word exactly once
 *   d_workspace  aesw_perm_workspace_bytes(n_sets) bytes, 16-byte aligned
 *   d_report     8-byte aligned; set by the call
 * k 17 ... 30 (2^k rows hold the table), n_sets 1 ... 1024, AESW_TABLE_ROWS <= n_rows <= 2^k, pad_row < AESW_TABLE_ROWS. */
int aesw_perm_build_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row,
                           const uint32_t *d_mult, uint32_t *d_a, uint32_t *d_s,
                           void *d_workspace, aesw_perm_report *d_report, void *stream);

/* d_out_fr[i] = d_table_fr[d_index[i]] for i < n_cells, 32 bytes each: the host's compressed table, any 32-byte values, gathered
 * through a column of row indices (d_a, d_s, or any part of them).  An index >= AESW_TABLE_ROWS gives a cell of 32 zero bytes
 * and reads nothing out of range.  d_index 4-byte, d_table_fr ([AESW_TABLE_ROWS][32]) and d_out_fr 16-byte aligned; n_cells up to
 * 2^36, 0: AESW_OK and nothing is launched.  The stores follow the context's "fr_store_mode", as aesw_expand_fr_device's. */
int aesw_perm_gather_fr_device(aesw_ctx *ctx, uint64_t n_cells, const uint32_t *d_index, const uint8_t *d_table_fr,
                               uint8_t *d_out_fr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_PERM_H */
