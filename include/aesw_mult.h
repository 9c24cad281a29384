/* aesw_mult.h -- C ABI of libaesw_mult.so: the lookup multiplicities of a many-circuit batch, counted on the device.
 *
 * The circuit has 5 * n_sets lookup arguments over 2^k rows each (src/aes128.rs:63-115), all into the 66 561-row table of
 * aesw_lookup_table (src/table.rs:18-192).  For every circuit c and column set s this library counts how often each table
 * row is looked up by the blocks Placement puts into set s of circuit c (set 0: and by the 400 rows of key slab c).  That is
 * the m column of a LogUp-style lookup argument, and what a plookup-style prover builds its permuted columns from by a
 * counting pass; no challenge is involved, so it belongs to witness generation.
 *
 * The bin of a lookup is the table row its INPUT operands name (aesw_mult_bin):
 *     tag 1 U8      x                       tag 4 GfMul2  66 048 + x
 *     tag 3 Sbox    256 + x                 tag 5 GfMul3  66 304 + x
 *     tag 2 Xor     512 + 256 x + y         row 66 560 (all zero): always 0
 * A lookup whose output is not what that row holds (y != sbox[x], z != x ^ y, ...; the tables are the context's) is counted
 * in no bin but in `misses`: misses == 0 is the lookup half of MockProver's criterion.  Rows without a lookup and rows no
 * block fills are not counted; the multiplicity of the all-zero row for the argument (set s, tag t) is
 * 2^k - (the sum of section t of histogram (c, s)).
 *
 * libaesw_mult.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_mult -laesw. */
#ifndef AESW_MULT_H
#define AESW_MULT_H

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aesw_mult_report {
    uint64_t lookups;     /* enabled lookups seen (hits + misses) */
    uint64_t misses;      /* enabled lookups with no table row */
    uint64_t first_miss;  /* AESW_CHECK_NONE, or the smallest miss, encoded like aesw_check_report.first
                             (unit = batch block index, or circuit index for a key slab; kind 1; index = slab row) */
} aesw_mult_report;

/* The arguments follow aesw_assemble_advice_circuits_device: circuit c owns blocks [offsets[c], offsets[c+1]) of the block
 * slabs d_x, d_y, d_z (`layout`: DENSE or PACKED; VALUES has no x: AESW_ERR_INVALID_ARG) and key slab c of d_key_slabs (ONE
 * aesw_key_slab whose columns hold C contiguous key slabs; NULL, or with kx, ky or kz NULL: no key lookups are counted; w is
 * not read).  For k < 9 no key lookups are counted either: 2^k rows do not hold the 400 key rows, and aesw_assemble_selectors
 * enables none of their selectors.  k 2 ... 30, n_sets 1 ... 1024, n_circuits >= 1 with n_circuits * n_sets <= 2^24.  d_x,
 * d_y, d_z and the key
 * columns are 16-byte aligned, d_offsets and d_report 8-byte.  A group context: AESW_ERR_INVALID_ARG.
 *
 * d_mult: [n_circuits][n_sets][AESW_TABLE_ROWS] uint32_t, 16-byte aligned.  32 bits hold every count: a set has 2^k <= 2^30
 * rows.  Histogram (c, s) covers the blocks of set s of circuit c; histogram (c, 0) also the key rows (160 U8, 200 Xor and
 * 40 Sbox lookups; words_column has no lookup).  The counts are exact for every input.
 *
 * The offsets are the caller's to validate, as for the assemble call: a count is clamped to aesw_block_capacity(k, n_sets),
 * so the kernel reads only inside each circuit's own range and writes only d_mult and d_report.
 *
 * The call sets all of d_mult and d_report itself, is asynchronous on `stream`, neither allocates nor waits on the host and
 * may be captured into a hipGraph: a replay counts again, it does not accumulate. */
int aesw_mult_count_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits,
                           const uint64_t *d_offsets, int layout,
                           const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z,
                           const aesw_key_slab *d_key_slabs,
                           uint32_t *d_mult, aesw_mult_report *d_report, void *stream);

/* The two forms of the count, byte-identical in result.  DIRECT: d_mult is zeroed and every lookup is one
 * global atomic add.  PRIVATE: two workgroups per (circuit, set) count in LDS -- one the Xor rows with x < 128 and the four
 * small sections, the other the Xor rows with x >= 128 -- and store their bins once, with plain contiguous stores. */
#define AESW_MULT_FORM_AUTO 0
#define AESW_MULT_FORM_DIRECT 1
#define AESW_MULT_FORM_PRIVATE 2

/* For tests and the bench tool: aesw_mult_count_device with the form forced (AUTO: what aesw_mult_count_device does). */
int aesw_mult_count_device_form(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits,
                                const uint64_t *d_offsets, int layout,
                                const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z,
                                const aesw_key_slab *d_key_slabs,
                                uint32_t *d_mult, aesw_mult_report *d_report, void *stream, int form);

/* Pure host: the form AUTO resolves to.  It depends on the shape alone, never on the counts. */
int aesw_mult_default_form(uint32_t k, uint32_t n_sets, uint32_t n_circuits);

/* Pure host: the bin rule above; UINT32_MAX for tag 0 and for anything that is no tag. */
uint32_t aesw_mult_bin(uint32_t tag, uint32_t x, uint32_t y);

#ifdef __cplusplus
}
#endif

#endif /* AESW_MULT_H */
