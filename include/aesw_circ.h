/* aesw_circ.h -- C ABI of libaesw_circ.so: MockProver's criterion over a many-circuit batch in one launch.
 *
 * The companion of aesw_assemble_advice_circuits_device (aesw.h "many circuits").  C FixedAes128Config<k, n_sets> circuits
 * lie in device memory as one batch: n block slabs (d_x, d_y, d_z in `layout`), C key slabs, and a DEVICE array d_offsets
 * of C+1 uint64_t in which circuit c owns blocks [offsets[c], offsets[c+1]).  aesw_check_witness_device (aesw.h) knows one
 * key slab for the whole batch or one per block; here block b is held against key slab circuit(b), every key slab is
 * checked once, and the offsets themselves are validated -- all by one kernel.
 *
 * libaesw_circ.so links against libaesw.so ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_circ -laesw. */
#ifndef AESW_CIRC_H
#define AESW_CIRC_H

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aesw_circ_check_report {
    uint64_t blocks;           /* block slabs checked: offsets[C] as the call was told (n) */
    uint64_t keys;             /* key slabs checked: C */
    uint64_t lookup_failures;  /* as in aesw_check_report */
    uint64_t copy_failures;
    uint64_t gate_failures;
    uint64_t input_failures;
    uint64_t first;            /* AESW_CHECK_NONE or the smallest failing check, macros of aesw.h;
                                  UNIT = batch-wide block index, or the circuit index for a key slab */
    uint64_t offset_failures;  /* circuits c with offsets[c+1] < offsets[c] or a count above
                                  aesw_block_capacity(k, n_sets), plus 1 if offsets[0] != 0, plus 1 if offsets[C] != n */
} aesw_circ_check_report;

/* Per block b < n: its 1 360 rows against the lookups, its 1 952 copies with the AddRoundKey edges resolved in key slab
 * circuit(b), rows 0..15 of x against d_pt and, when d_ct is given, the last xor rows against it.  Per key slab c < C
 * (circuits without a block included): 400 rows, 640 copies, the round-constant gate, and words_column rows 0..15 against
 * d_keys + 16 c when d_keys is given.  Exactly what aesw_check_witness_device checks per unit.
 *
 * layout: DENSE or PACKED (VALUES: AESW_ERR_INVALID_ARG).  k 2 ... 30, n_sets 1 ... 1024, n_circuits >= 1.  The columns
 * (d_x, d_y, d_z, the four of d_key_slabs) are 16-byte aligned, d_pt / d_ct / d_keys 4-byte, d_offsets and d_report 8-byte.
 * d_key_slabs (REQUIRED): ONE aesw_key_slab whose columns hold C contiguous key slabs, as for the assemble call.  n == 0 is
 * legal (d_pt, d_x, d_y, d_z may then be NULL): the C key slabs are still checked.  A group context: AESW_ERR_INVALID_ARG.
 *
 * Offsets that break the rules (offsets[0] = 0, non-decreasing, offsets[C] = n, counts within the capacity) are COUNTED in
 * offset_failures, exactly, and never move a read outside the batch: every block index stays below n, and a block is held
 * against key slab aesw_circ_circuit_of_block(offsets, C, b), which lies in [0, C) whatever the offsets hold.  The other
 * failure counts are unspecified for such offsets.
 *
 * The report is reset on `stream` by the call (a small launch of its own) and written by the kernel; read it back after
 * synchronising.  The call is asynchronous, neither allocates nor waits on the host, and may be captured into a hipGraph. */
int aesw_circ_check_witness_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits,
                                   const uint64_t *d_offsets, uint64_t n,
                                   const uint8_t *d_pt, const uint8_t *d_keys /* C * 16, or NULL */,
                                   int layout, const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z,
                                   const uint8_t *d_ct /* n * 16, or NULL */,
                                   const aesw_key_slab *d_key_slabs /* C contiguous slabs, REQUIRED */,
                                   aesw_circ_check_report *d_report, void *stream);

/* Pure host: the circuit the kernel holds block b against, from a HOST copy of the offsets (n_circuits + 1 entries, of which
 * only [1, n_circuits) are read).  For valid offsets and b < offsets[n_circuits] it is the c with offsets[c] <= b <
 * offsets[c+1]; for any offsets it lies in [0, n_circuits).  Returns 0 for n_circuits == 0 or offsets == NULL. */
uint32_t aesw_circ_circuit_of_block(const uint64_t *offsets, uint32_t n_circuits, uint64_t b);

#ifdef __cplusplus
}
#endif

#endif /* AESW_CIRC_H */
