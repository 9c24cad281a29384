/* aesw_ntt.h -- C ABI of libaesw_ntt.so: columns of Fr cells between Lagrange, coefficient and extended-coset form, on the device.
 *
 * halo2's prover holds a column as its 2^k evaluations on {omega_k^i} (Lagrange form), turns it into the 2^k coefficients of the
 * polynomial through them (lagrange_to_coeff), evaluates that on the coset zeta * {omega_ext^i} of a larger domain
 * (coeff_to_extended), works there, and comes back (extended_to_coeff).  These are number-theoretic transforms over bn256's scalar
 * field, with omega_k = g^((r - 1) / 2^k) and g = 7 the generator:
 *   coeff_to_lagrange      out[j] = sum_i in[i] * omega_k^(i j)                                    (halo2: best_fft with omega_k)
 *   lagrange_to_coeff      its inverse: out[i] = 2^-k * sum_j in[j] * omega_k^(-i j)
 *   coeff_to_extended      out[j] = sum_(i < 2^k) in[i] * zeta^(i mod 3) * omega_ext^(i j),  j < 2^ext_k
 *   extended_to_coeff      its inverse over all 2^ext_k coefficients: out[i] = zeta^-(i mod 3) * 2^-ext_k * sum_j in[j] * omega_ext^(-i j)
 *                          (halo2 truncates the result afterwards; this call does not)
 *
 * A COLUMN is 2^k cells of 32 bytes, columns lie one behind the other ([n_cols][2^k][32]), 16-byte aligned.  A CELL is eight
 * little-endian 32-bit limbs of v * 2^256 mod r -- the Montgomery form of every Fr cell of aesw.h.  Input and output are in natural
 * order on both sides of every call.  n_cols * 2^k may pass 2^27 cells (4 GiB): every offset is 64 bits.
 *
 * ZETA: zeta_sel 0 is g^((r - 1) / 3), zeta_sel 1 its square; both are derived, none is quoted.  Which of the two halo2curves
 * calls Fr::ZETA is NOT PINNED by a test here -- from memory it is the square, zeta_sel 1 (0x3064...636f23).  The coefficients a
 * round trip through the extended domain gives do not depend on the choice; only a host that mixes extended arrays with halo2's
 * own is affected.
 *
 * NON-CANONICAL INPUT CELLS (values at or above r): the output VALUES are unspecified; the call still writes only its outputs, and
 * all of them.  Every producer of Fr cells in this project writes canonical cells, and there is no report.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, uses no atomic -- the passes of
 * a transform are ordered by the stream -- and may be captured into a hipGraph: a replay transforms what the input then holds.
 * A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and the outputs untouched; aesw_last_error names the call.  A
 * group context is refused.  Bounds: 10 <= k <= ext_k <= max_k <= 28 (the field's 2-adicity), 1 <= n_cols <= 65535.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_ntt -laesw. */
#ifndef AESW_NTT_H
#define AESW_NTT_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_tables for transforms up to 2^max_k: about 1 MiB at 28; 0 outside 10 ... 28.  A multiple of 16. */
size_t aesw_ntt_tables_bytes(uint32_t max_k);

/* Bytes of d_workspace for a transform of size 2^k over n_cols columns: one copy of the columns where the transform takes more
 * than one pass (k > 10), else 0; 0 outside the bounds.  A multiple of 16.  Only a call whose output IS its input uses it -- any
 * other call may pass NULL; two calls in flight need two. */
size_t aesw_ntt_workspace_bytes(uint32_t k, uint32_t n_cols);

/* The twiddle tables, once per max_k: d_tables (16-byte aligned, aesw_ntt_tables_bytes) serves every transform of size up to
 * 2^max_k.  It holds the powers of omega_10 (the roots of a pass), omega_max_k^j for j < 2^min(max_k, 14) and
 * omega_max_k^(j * 2^14) for j < 2^max(max_k - 14, 0), and 2^-k * zeta0^v for k <= 28, v < 3.  A transform whose output overlaps
 * the tables is refused. */
int aesw_ntt_tables_device(aesw_ctx *ctx, uint32_t max_k, uint8_t *d_tables, void *stream);

/* Evaluations on {omega_k^i} -> coefficients (halo2's lagrange_to_coeff; includes the 1/2^k).  d_in == d_out is allowed (then
 * d_workspace must be there where aesw_ntt_workspace_bytes is not 0); any other overlap is refused.  Stores of the result follow
 * the context's "fr_store_mode". */
int aesw_ntt_lagrange_to_coeff_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_in, uint8_t *d_out,
                                      const uint8_t *d_tables, uint32_t max_k, void *d_workspace, void *stream);

/* Its inverse: coefficients -> evaluations on {omega_k^i}.  Same arguments, same rules. */
int aesw_ntt_coeff_to_lagrange_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_in, uint8_t *d_out,
                                      const uint8_t *d_tables, uint32_t max_k, void *d_workspace, void *stream);

/* 2^k coefficients -> 2^ext_k evaluations on zeta * {omega_ext^i} (halo2's coeff_to_extended): coefficient i times
 * (1, zeta, zeta^2)[i mod 3], zero padding, forward transform of size 2^ext_k.  d_coeff [n_cols][2^k][32], d_ext
 * [n_cols][2^ext_k][32]; the two must not overlap.  d_workspace is not used and may be NULL. */
int aesw_ntt_coeff_to_extended_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_cols,
                                      const uint8_t *d_coeff, uint8_t *d_ext, const uint8_t *d_tables, uint32_t max_k,
                                      void *d_workspace, void *stream);

/* Its inverse: 2^ext_k evaluations on the coset -> 2^ext_k coefficients (halo2's extended_to_coeff without the truncation): of
 * what coeff_to_extended made, the 2^k coefficients followed by zeros.  d_ext == d_coeff is allowed, with d_workspace sized for
 * (ext_k, n_cols); any other overlap is refused. */
int aesw_ntt_extended_to_coeff_device(aesw_ctx *ctx, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_cols, const uint8_t *d_ext,
                                      uint8_t *d_coeff, const uint8_t *d_tables, uint32_t max_k, void *d_workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_NTT_H */
