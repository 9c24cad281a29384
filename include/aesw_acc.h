/* aesw_acc.h -- C ABI of libaesw_acc.so: the lookup multiplicities of ONE circuit, accumulated chunk by chunk on the device.
 *
 * aesw_mult_count_device (aesw_mult.h) needs the whole many-circuit batch resident and sets all of d_mult in one call.  A host
 * that generates a circuit's blocks piece by piece -- the chunked stream, or any loop that reuses its slab buffers -- never
 * holds such a batch.  Here the host resets a circuit's histograms once and then adds any contiguous run of the circuit's
 * blocks to them, in any number of calls and in any order; the result is what the one-shot call gives over the whole circuit:
 * integer adds commute, so neither the order of the calls nor how a range is cut enters.
 *
 * The bins, the hits and the misses are those of aesw_mult.h (the bin of a lookup is the table row its INPUT operands name; a
 * lookup whose output is not what that row holds is counted in no bin but in `misses`), and the report is its
 * aesw_mult_report: this header includes aesw_mult.h for the struct only, libaesw_mult.so is not needed.
 *
 * Every call is asynchronous on `stream`, neither allocates nor waits on the host and may be captured into a hipGraph; a
 * replay of captured adds adds again.  k 2 ... 30, n_sets 1 ... 1024; d_mult is 16-byte aligned, d_report 8-byte, d_x, d_y, d_z
 * and the key columns 16-byte.  A group context and a VALUES layout: AESW_ERR_INVALID_ARG, with the call named in
 * aesw_last_error.
 *
 * libaesw_acc.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_acc -laesw. */
#ifndef AESW_ACC_H
#define AESW_ACC_H

#include "aesw_mult.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_mult: [n_sets][AESW_TABLE_ROWS] uint32_t -- histogram (c, .) of aesw_mult_count_device for ONE circuit -- set to zero;
 * d_report to (0 lookups, 0 misses, AESW_CHECK_NONE). */
int aesw_acc_reset_device(aesw_ctx *ctx, uint32_t n_sets, uint32_t *d_mult, aesw_mult_report *d_report, void *stream);

/* Adds the lookups of blocks [first_block, first_block + n_blocks) of one FixedAes128Config<k, n_sets> circuit.  d_x, d_y, d_z
 * hold exactly those n_blocks slabs (slab i = circuit block first_block + i; `layout`: DENSE or PACKED); the set a block is
 * counted into is the one the circuit places it in (aesw_block_placement).  first_block + n_blocks >
 * aesw_block_capacity(k, n_sets): AESW_ERR_CAPACITY, nothing is enqueued.  n_blocks == 0: AESW_OK, nothing is launched.
 * d_report: `lookups` and `misses` grow by what this call saw; `first_miss` becomes the smaller of what it was and this call's
 * smallest miss, encoded as in aesw_mult_report with unit = the CIRCUIT's block index first_block + i. */
int aesw_acc_add_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, int layout,
                        const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z,
                        uint32_t *d_mult, aesw_mult_report *d_report, void *stream);

/* Adds the 400 key rows of ONE key slab (kx, ky, kz in `layout`, DENSE or PACKED -- a key slab's columns differ between the
 * two as a block's do; w is not read) to histogram 0: 160 U8, 200 Xor and 40 Sbox lookups.  A miss names unit 0 with the
 * key-slab bit set.  k < 9: AESW_OK and nothing is counted -- 2^k rows do not hold the key rows and
 * aesw_assemble_selectors enables none of their selectors (as aesw_mult_count_device). */
int aesw_acc_add_key_device(aesw_ctx *ctx, uint32_t k, int layout, const aesw_key_slab *d_key_slab,
                            uint32_t *d_mult, aesw_mult_report *d_report, void *stream);

/* For tests and the bench tool: aesw_acc_add_device with the blocks one pair of workgroups takes forced (at most 2^22 pairs per
 * column set); 0: the default, aesw_acc_default_chunk. */
int aesw_acc_add_device_chunk(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, int layout,
                              const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z,
                              uint32_t *d_mult, aesw_mult_report *d_report, void *stream, uint32_t blocks_per_workgroup);

/* Pure host: the blocks one pair of workgroups takes by default.  It depends on the shape alone, never on the counts, and is
 * at least 1. */
uint32_t aesw_acc_default_chunk(uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks);

#ifdef __cplusplus
}
#endif

#endif /* AESW_ACC_H */
