/* aesw_vals.h -- C ABI of libaesw_vals.so: MockProver's criterion over a VALUES witness, in one check launch.
 *
 * AESW_LAYOUT_VALUES holds only the cells a chip's closure computes: per block 448 y bytes (S-box and mul rows) and 608 z bytes
 * (xor rows), no x column.  aesw_check_witness_device (aesw.h) and aesw_circ_check_witness_device (aesw_circ.h) refuse it.
 * Every cell it leaves out is the destination of a copy_advice() or a plaintext literal, so a host that keeps the reference's
 * chips fills those cells by copying, and the full assignment is determined by the plaintext, the round-key cells of the key
 * slab and the VALUES bytes.  On that assignment every copy of a block holds by construction; what is left to check are the
 * 1 056 enabled lookups of a block -- 160 S-box, 144 mul2, 144 mul3, 608 xor -- with every x, and the y of an xor row, resolved
 * through aesw_block_copy_graph to the cell it ultimately copies from, and the key slab(s), which VALUES keeps in PACKED form.
 *
 * THE IMAGE.  Offsets of the table below address one unit's bytes in this order:
 *     y  [0, 448)         the block's VALUES y bytes           (aesw_layout_index(AESW_LAYOUT_VALUES, 1, ..))
 *     z  [448, 1056)      the block's VALUES z bytes           (aesw_layout_index(AESW_LAYOUT_VALUES, 2, ..))
 *     pt [1056, 1072)     the block's plaintext
 *     kx [1072, 1472) | ky [1472, 1712) | kz [1712, 1912) | words_column [1912, 2008)     the PACKED key slab
 * THE TABLE.  One entry of two words per slab row whose tag (aesw_selector_tags) is >= 2, in row order:
 *     words[2 e] = ox | oy << 16,   words[2 e + 1] = oz | tag << 16,   rows[e] = the slab row
 * ox / oy: image offset of the cell the row's x / y resolves to -- a VALUES cell, a plaintext byte, or one of the 176
 * round-key cells (words_column rows 0..15, 160 kz cells); for a tag >= 3 oy is the row's own y cell.  oz: the row's own z cell
 * for an xor row, 0xffff (unused) otherwise.  An xor row holds when z == x ^ y, a tag >= 3 row when y == table[tag - 3][x].
 *
 * libaesw_vals.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_vals -laesw. */
#ifndef AESW_VALS_H
#define AESW_VALS_H

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aesw_check_witness_device for a VALUES witness: no `layout`, no d_x.  d_y / d_z: n * 448 / n * 608 bytes as
 * aesw_encrypt_witness_device writes them for AESW_LAYOUT_VALUES; d_key_slab: REQUIRED, packed -- one key slab, or n with
 * per_block_keys; for a scheduled key the slab aesw_schedule_key_device wrote.  d_keys: 16 bytes, n * 16 with per_block_keys,
 * or NULL without (the key literal is then not compared).  d_ct: n * 16 or NULL; when given, the last sixteen z cells of every
 * block are compared with it (AESW_CHECK_INPUT at rows 1344..1359).
 *
 * The report is aesw_check_report, read with the AESW_CHECK_* macros: lookup failures of a block at their slab row;
 * copy_failures and gate_failures can only come from key slabs; a block has no plaintext literal check (its plaintext is an
 * input of the lookups that read it).  The counts equal those of aesw_check_witness_device over the PACKED witness that
 * copying produces from the same bytes.  blocks = n; keys = n with per_block_keys, else 1 (a shared key slab is checked once).
 *
 * d_y, d_z, d_pt, d_ct and the four key-slab columns are 16-byte aligned (a block travels as 16-byte loads), d_keys 4-byte,
 * d_report 8-byte.  n == 0 is legal (d_pt / d_y / d_z may then be NULL): the report is reset and nothing is checked.  A group
 * context: AESW_ERR_INVALID_ARG.  The report is reset on `stream` by a small launch of the call's own and written by the
 * kernel; nothing else is written.  The call is asynchronous, neither allocates nor waits on the host, and may be captured
 * into a hipGraph -- with one exception: the first call on a device copies the 24 KiB check table into the library's own
 * device storage, synchronously.  aesw_vals_prepare() does that ahead of time. */
int aesw_vals_check_device(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n,
                           const uint8_t *d_y, const uint8_t *d_z, const uint8_t *d_ct,
                           const aesw_key_slab *d_key_slab /* REQUIRED, packed */, aesw_check_report *d_report, void *stream);

/* Uploads the check table to the context's device if this process has not done so yet (idempotent, thread-safe). */
int aesw_vals_prepare(aesw_ctx *ctx);

/* Pure host: the number of checked rows of a block, 1 056. */
uint32_t aesw_vals_check_rows(void);
/* Pure host: the table described above.  words: 2 * aesw_vals_check_rows() entries, rows: aesw_vals_check_rows(); either may
 * be NULL. */
int aesw_vals_check_table(uint32_t *words, uint16_t *rows);
/* Pure host: bytes of the image the offsets address, 2 008. */
uint32_t aesw_vals_image_bytes(void);

#ifdef __cplusplus
}
#endif

#endif /* AESW_VALS_H */
