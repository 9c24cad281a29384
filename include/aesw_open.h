/* aesw_open.h -- C ABI of libaesw_open.so: columns of Fr cells in coefficient form evaluated at points, folded under a challenge
 * and divided by (X - z), on the device.
 *
 * After its last challenge halo2's prover evaluates every queried polynomial at x * omega^rot (eval_polynomial), folds the
 * polynomials opened at one point under v, and commits to the quotient of each fold by (X - z) (kate_division).  For a column of
 * coefficients c_0 ... c_(n-1), n = 2^k, and a point z, with S_n = 0 and S_i = c_i + z * S_(i+1):
 *   evaluate   p(z) = sum_i c_i z^i = S_0
 *   divide     (p(X) - p(z)) / (X - z) has the coefficients q[i] = S_(i+1), i < n - 1, and q[n-1] = 0; the remainder is p(z)
 *   fold       folded[i] = (...((acc[i] * v + col_0[i]) * v + col_1[i])...) * v + col_(n_cols-1)[i]
 * The fold's order is that of halo2 v0.3.0's GWC prover restated from memory: acc = acc * v + poly, the first column of a point
 * first.  It is NOT PINNED by a test here; a host that needs another order folds column by column in the order it needs
 * (d_acc_in == d_folded).
 *
 * A COLUMN is 2^k cells of 32 bytes, columns lie one behind the other ([n_cols][2^k][32]), 16-byte aligned.  A CELL is eight
 * little-endian 32-bit limbs of v * 2^256 mod r -- the Montgomery form of every Fr cell of aesw.h; what the transform library
 * writes in coefficient form is taken as it lies.  n_cols * 2^k may pass 2^27 cells (4 GiB): every offset is 64 bits.
 *
 * POINTS and v are cells in DEVICE memory (16-byte aligned, Montgomery form), read when the kernels run: a captured call
 * follows them, as the grand products follow d_beta.  z = 0 is a point like any other.
 *
 * NON-CANONICAL INPUT CELLS (values at or above r), points and v among them: the output VALUES are unspecified; the call still
 * writes only its outputs, and all of them.  Every producer of Fr cells in this project writes canonical cells, and there is no
 * report.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, uses no atomic -- the passes of
 * a call are ordered by the stream -- and may be captured into a hipGraph.  A refusal returns AESW_ERR_INVALID_ARG with nothing
 * enqueued and the outputs untouched; aesw_last_error names the call and the argument.  A group context is refused.
 * Bounds: 10 <= k <= 28, 1 <= n_cols <= 65535, 1 <= n_points <= 16.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_open -laesw. */
#ifndef AESW_OPEN_H
#define AESW_OPEN_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of d_workspace for n_cols columns of 2^k cells at n_points points (a division has one): 29 cells per point -- the powers
 * z^(2^s) -- and one cell per chunk of 1 024 coefficients, column and point; 0 outside the bounds.  A multiple of 16.  Two calls
 * in flight need two. */
size_t aesw_open_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t n_points);

/* d_evals[c][p] = sum_i d_coeff[c][i] * z_p^i: every column at every point, the column read once.  d_coeff [n_cols][2^k][32],
 * d_points [n_points][32], d_evals [n_cols][n_points][32], d_workspace aesw_open_workspace_bytes(k, n_cols, n_points); no two of
 * them may overlap. */
int aesw_open_evaluate_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t n_points, const uint8_t *d_coeff, const uint8_t *d_points,
                              uint8_t *d_evals, void *d_workspace, void *stream);

/* d_folded[i] = (...((acc[i] * v + col_0[i]) * v + col_1[i])...) * v + col_(n_cols-1)[i], i < 2^k, the n_cols columns of d_coeff
 * in their order; acc is d_acc_in [2^k][32], or zero where d_acc_in is NULL.  d_acc_in == d_folded is allowed, so columns that
 * live in separate allocations are folded by successive calls; any other overlap of d_folded is refused.  d_v: one cell.  Stores
 * of the result follow the context's "fr_store_mode". */
int aesw_open_fold_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_v, const uint8_t *d_acc_in,
                          uint8_t *d_folded, void *stream);

/* For every column: d_quot[c] the 2^k coefficients of (p_c(X) - p_c(z)) / (X - z) -- the last one 0 -- and d_rem[c] = p_c(z).  One
 * point, d_point [32].  d_quot [n_cols][2^k][32] may be d_coeff itself (the columns are divided in place); a partial overlap is
 * refused.  d_rem [n_cols][32], d_workspace aesw_open_workspace_bytes(k, n_cols, 1); neither may overlap anything else.  Stores of
 * the quotient follow the context's "fr_store_mode". */
int aesw_open_divide_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_point, uint8_t *d_quot,
                            uint8_t *d_rem, void *d_workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_OPEN_H */
