/* aesw_vacc.h -- C ABI of libaesw_vacc.so: the lookup multiplicities of ONE circuit accumulated from a VALUES witness.
 *
 * AESW_LAYOUT_VALUES holds per block 448 y and 608 z bytes and no x column (aesw_vals.h).  aesw_acc_add_device (aesw_acc.h) and
 * aesw_mult_count_device (aesw_mult.h) refuse it: they read the operands of a lookup on the lookup's own row.  A host that keeps
 * the reference's chips fills the cells VALUES leaves out by copying, so every operand is determined by the VALUES bytes, the
 * plaintext and the 176 round-key cells of the key slab; this library reads each operand where the copies end -- the table of
 * aesw_vals_check_table (aesw_vals.h) -- and counts the block's 1 056 lookups from 1 072 bytes instead of 3 024.
 *
 * THE HISTOGRAMS AND THE REPORT ARE aesw_acc.h's.  d_mult is its [n_sets][AESW_TABLE_ROWS] uint32_t, reset by its
 * aesw_acc_reset_device; the key slab's own 400 rows are added by its aesw_acc_add_key_device(..., AESW_LAYOUT_PACKED, ...), since
 * the key slabs of VALUES are the packed ones.  One set of histograms takes VALUES adds, PACKED adds and the key add in any
 * order.  The bins, the hits and the misses are those of aesw_mult.h, and the report is its aesw_mult_report: this header
 * includes aesw_mult.h for the struct only, neither libaesw_mult.so nor libaesw_acc.so is needed by this library.
 *
 * THE RESULT is what aesw_acc_add_device gives over the PACKED witness that copying produces from the same bytes, corrupted
 * bytes included: a wrong VALUES cell is a miss on its own row, and whatever hit or miss it makes of every row that reads it.
 *
 * Every add is asynchronous on `stream`, neither allocates nor waits on the host and may be captured into a hipGraph (a replay
 * of captured adds adds again) -- with one exception: the first add on a device copies the 10 KiB table into the library's own
 * device storage, synchronously.  aesw_vacc_prepare() does that ahead of time.  k 2 ... 30, n_sets 1 ... 1024; d_pt, d_y, d_z and
 * the key slab's kz and w are 16-byte aligned, d_mult 16-byte, d_report 8-byte.  A group context: AESW_ERR_INVALID_ARG, with the
 * call named in aesw_last_error.
 *
 * libaesw_vacc.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_vacc -laesw (and -laesw_acc for the reset and the key add). */
#ifndef AESW_VACC_H
#define AESW_VACC_H

#include "aesw_mult.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Adds the lookups of blocks [first_block, first_block + n_blocks) of one FixedAes128Config<k, n_sets> circuit, given as a
 * VALUES witness.
 *   d_pt         n_blocks * 16 plaintext bytes
 *   d_y / d_z    n_blocks * 448 / n_blocks * 608 bytes, as aesw_encrypt_witness_device writes them for AESW_LAYOUT_VALUES
 *   d_key_slab   REQUIRED: the circuit's ONE packed key slab.  Only its kz and words_column (w) are read, the 176 round-key
 *                cells.
 * Slab i is circuit block first_block + i; the set a block is counted into is the one the circuit places it in
 * (aesw_block_placement).  first_block + n_blocks > aesw_block_capacity(k, n_sets): AESW_ERR_CAPACITY, nothing is enqueued.
 * n_blocks == 0: AESW_OK, nothing is launched.  d_report: `lookups` grows by 1 056 per block, `misses` by what this call saw;
 * `first_miss` becomes the smaller of what it was and this call's smallest miss, encoded as in aesw_mult_report with unit =
 * the CIRCUIT's block index first_block + i and the SLAB row of the lookup (0 ... 1 359), as aesw_acc_add_device names it. */
int aesw_vacc_add_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks,
                         const uint8_t *d_pt, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slab,
                         uint32_t *d_mult, aesw_mult_report *d_report, void *stream);

/* For tests and the bench tool: the same with the blocks one pair of workgroups takes forced (at most 2^22 pairs per column
 * set); 0: the default, aesw_vacc_default_chunk. */
int aesw_vacc_add_device_chunk(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks,
                               const uint8_t *d_pt, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slab,
                               uint32_t *d_mult, aesw_mult_report *d_report, void *stream, uint32_t blocks_per_workgroup);

/* Pure host: the blocks one pair of workgroups takes by default.  It depends on the shape alone, never on the counts, is at
 * least 1 and equals aesw_acc_default_chunk. */
uint32_t aesw_vacc_default_chunk(uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks);

/* Uploads the library's table to the context's device if this process has not done so yet (idempotent, thread-safe). */
int aesw_vacc_prepare(aesw_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* AESW_VACC_H */
