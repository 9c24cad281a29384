/* aesw_cols.h -- C ABI of libaesw_cols.so: MockProver's criterion over the ASSEMBLED advice columns of a many-circuit batch,
 * as bytes or as bn256::Fr cells, in one launch.
 *
 * aesw_check_witness_device (aesw.h) and aesw_circ_check_witness_device (aesw_circ.h) certify witness slabs.  The prover
 * takes the columns aesw_assemble_advice_device / aesw_assemble_advice_circuits_device build from them: C circuits of
 * (3 n_sets + 1) << k cells each, one byte or AESW_FR_BYTES per cell.  The call below holds those columns against the same
 * checks -- every enabled lookup, every copy_advice() pair, the round-constant gate, the literal rows -- and against the two
 * properties only the assembled form has: every cell the reference never assigns is 0, and every Fr cell is exactly the
 * Montgomery form of a byte.
 *
 * libaesw_cols.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_cols -laesw. */
#ifndef AESW_COLS_H
#define AESW_COLS_H

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aesw_cols_check_report {
    uint64_t blocks;               /* blocks checked: n as the call was told */
    uint64_t keys;                 /* key-row units checked: C */
    uint64_t lookup_failures;      /* as in aesw_check_report */
    uint64_t copy_failures;
    uint64_t gate_failures;
    uint64_t input_failures;
    uint64_t first;                /* AESW_CHECK_NONE or the smallest failing check, macros of aesw.h; UNIT = batch-wide
                                      block index, or the circuit index for the key rows */
    uint64_t offset_failures;      /* exactly as in aesw_circ_check_report */
    uint64_t cell_failures;        /* as_fr only: cells whose 32 bytes are not the Montgomery form of some byte 0..255 */
    uint64_t unassigned_failures;  /* cells the reference never assigns that are not 0 (as_fr: not 32 zero bytes) */
    uint64_t first_cell;           /* UINT64_MAX, or the smallest absolute cell index in d_cols counted in either of the
                                      two above (aesw_cols_cell_index) */
    uint64_t cells;                /* cells examined: C * (3 n_sets + 1) << k */
} aesw_cols_check_report;

/* d_cols: exactly what aesw_assemble_advice_circuits_device writes (as_fr as there); C = 1 with offsets {0, n} is the output
 * of aesw_assemble_advice_device.  Circuit c's local block j is block offsets[c] + j of the batch: it lies where
 * aesw_block_placement(k, n_sets, j) says, is held against rows 0..399 of set 0 and words_column rows 0..95 of the same
 * circuit, and d_pt + 16 (offsets[c] + j) / d_ct are its literals.  The key rows of every circuit are checked once, circuits
 * without a block included, as aesw_check_witness_device checks a key slab (d_keys: C * 16 bytes or NULL).
 *
 * A cell is NEVER ASSIGNED when no assigned cell of a DENSE slab maps to it: the y / z cells of slab rows the reference
 * leaves out, every row behind a circuit's last block in every column set, words_column from row 96 on.  Every cell of the
 * matrix is examined exactly once for cell_failures / unassigned_failures, and both counts are exact.  A never-assigned
 * cell that is not canonical counts in both.  For a unit that holds a non-canonical Fr cell the byte taken for that cell is
 * unspecified, and with it the unit's lookup / copy / gate / input counts and `first`.
 *
 * Offsets that break the rules of aesw_circ.h are counted in offset_failures as there (a count is clamped to the capacity
 * where rows are swept) and never move a read outside d_cols, d_pt or d_ct; the other counts are then unspecified.
 *
 * k 9 ... 30 (the 400 key rows must fit), n_sets 1 ... 1024, n_circuits >= 1 with n_circuits (3 n_sets + 1) < 2^32; n == 0 is
 * legal (d_pt may then be NULL).  d_cols is 16-byte aligned, d_pt / d_ct / d_keys 4-byte, d_offsets and d_report 8-byte.
 * A group context: AESW_ERR_INVALID_ARG.  The report is reset on `stream` by a small launch of the call's own and written
 * by the kernel.  The call is asynchronous, neither allocates nor waits on the host, and may be captured into a hipGraph. */
int aesw_cols_check_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits,
                           const uint64_t *d_offsets, uint64_t n,
                           const uint8_t *d_pt, const uint8_t *d_keys /* C * 16, or NULL */,
                           const uint8_t *d_ct /* n * 16, or NULL */,
                           int as_fr, const uint8_t *d_cols, aesw_cols_check_report *d_report, void *stream);

/* Pure host: the absolute cell index `first_cell` uses: ((circuit (3 n_sets + 1) + column) << k) + row. */
uint64_t aesw_cols_cell_index(uint32_t k, uint32_t n_sets, uint32_t circuit, uint32_t column, uint64_t row);

/* Pure host: the 256 x 32-byte table byte -> bn256::Fr (little-endian Montgomery form) the library searched its hash for. */
void aesw_cols_fr_table(uint8_t table[256 * 32]);

/* Pure host: how the kernel takes an Fr cell back to its byte without field arithmetic.  The search looks for an odd
 * multiplier `mul` and a width `bits` (8 ... 12, the smallest that works) such that  (low dword * mul) >> (32 - bits)  is
 * injective over the 256 entries of `table`; inv (1 << 12 bytes) then maps that value to the byte (unused slots: 0).
 * Returns AESW_OK, or AESW_ERR_INVALID_ARG when no such pair was found (the library then refuses every as_fr call). */
int aesw_cols_hash_search(const uint8_t table[256 * 32], uint32_t *mul, uint32_t *bits, uint8_t inv[4096]);
/* The byte whose table entry equals all 32 bytes of `cell`, found through the hash; -1 if there is none. */
int aesw_cols_hash_invert(const uint8_t table[256 * 32], uint32_t mul, uint32_t bits, const uint8_t inv[4096],
                          const uint8_t cell[32]);

#ifdef __cplusplus
}
#endif

#endif /* AESW_COLS_H */
