/* Certify the assembled advice columns of C circuits on the device, in the form handed to create_proof (include/aesw_cols.h).
 *
 *   cc -Iinclude examples/aesw_cols_check.c -Lhalo2-aes_amd -laesw_cols -laesw -L/opt/rocm/lib -lamdhip64
 *
 * The caller has d_cols from aesw_assemble_advice_circuits_device (as_fr as there), the batch's plaintexts, keys and
 * ciphertexts, and the device offsets; the report is read back after synchronising the stream. */
#include <stdio.h>

#include "aesw_cols.h"

int certify_columns(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, uint64_t n,
                    const uint8_t *d_pt, const uint8_t *d_keys, const uint8_t *d_ct, int as_fr, const uint8_t *d_cols,
                    aesw_cols_check_report *d_report, void *stream) {
    int rc = aesw_cols_check_device(ctx, k, n_sets, n_circuits, d_offsets, n, d_pt, d_keys, d_ct, as_fr, d_cols, d_report, stream);
    if (rc != AESW_OK) fprintf(stderr, "aesw_cols_check_device: %s (%s)\n", aesw_strerror(rc), aesw_last_error(ctx));
    return rc;
}

/* after the stream is synchronised and the report copied to the host */
int columns_satisfied(const aesw_cols_check_report *r, uint32_t k, uint32_t n_sets) {
    if (r->lookup_failures | r->copy_failures | r->gate_failures | r->input_failures | r->offset_failures) {
        if (r->first != AESW_CHECK_NONE)
            fprintf(stderr, "first failing check: unit %llu%s kind %u index %u\n", (unsigned long long)AESW_CHECK_UNIT(r->first),
                    AESW_CHECK_IS_KEY_SLAB(r->first) ? " (key rows)" : "", (unsigned)AESW_CHECK_KIND(r->first), (unsigned)AESW_CHECK_INDEX(r->first));
        return 0;
    }
    if (r->cell_failures | r->unassigned_failures) {
        const uint64_t per_circuit = (uint64_t)(3 * n_sets + 1) << k;
        const uint64_t c = r->first_cell / per_circuit, rest = r->first_cell % per_circuit;
        fprintf(stderr, "first bad cell: circuit %llu column %llu row %llu (cell %llu = %llu)\n", (unsigned long long)c,
                (unsigned long long)(rest >> k), (unsigned long long)(rest & (((uint64_t)1 << k) - 1)), (unsigned long long)r->first_cell,
                (unsigned long long)aesw_cols_cell_index(k, n_sets, (uint32_t)c, (uint32_t)(rest >> k), rest & (((uint64_t)1 << k) - 1)));
        return 0;
    }
    return r->cells == (((uint64_t)r->keys * (3 * n_sets + 1)) << k);
}
