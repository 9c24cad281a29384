/* aesw_quot.h -- C ABI of libaesw_quot.so: sigma of the permutation argument written out as Fr columns, on the device -- the one
 * input of the quotient h(X) of a FixedAes128Config<k, n_sets> circuit (halo2's evaluate_h) that no other library of the project
 * writes.  The evaluation of the quotient itself is NOT part of this library yet: its rules and its fold are stated and tested on
 * the CPU (csrc/aesw_quot.h), its kernel is left out.
 *
 * A CELL is eight little-endian 32-bit limbs of v * 2^256 mod r, the Montgomery form of every Fr cell of aesw.h.  The labels are
 * delta^c' * omega_k^i' with omega_k = g^((r - 1) / 2^k), delta = g^(2^28) and g = 7, as the permutation library derives them.
 *
 * THE ORDER of the permutation's columns and the mapping are the permutation library's; parity of that mapping with halo2's own
 * keygen is NOT PINNED by a test there, and so neither is parity of these columns with halo2's permutation polynomials.
 *
 * The device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, uses no atomic and may be captured
 * into a hipGraph.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and the output untouched; aesw_last_error names the
 * call.  A group context is refused.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_quot -laesw. */
#ifndef AESW_QUOT_H
#define AESW_QUOT_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sigma as cells, the Lagrange form of halo2's permutation polynomials: d_sigma_fr[c][i] ([n_cols][2^k][32]) is the label
 * delta^c' * omega^i' of the cell d_map[c][i] = c' * 2^k + i' ([n_cols][2^k] uint32_t, the permutation library's mapping).  An entry
 * at or above n_cols * 2^k reads as the cell itself.  d_sigma_tables: the power tables the permutation library writes for the same
 * (k, n_cols).  Bounds: that library's, 10 <= k <= 28, 1 <= n_cols <= 3074, n_cols * 2^k <= 2^32.  Every pointer 16-byte aligned.
 * The caller moves the result to coefficient form and onto the coset with the transforms.  The output must not overlap the inputs. */
int aesw_quot_sigma_fr_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint32_t *d_map, const uint8_t *d_sigma_tables,
                              uint8_t *d_sigma_fr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_QUOT_H */
