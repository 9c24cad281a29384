/* aesw_msm.h -- C ABI of libaesw_msm.so: columns of scalars committed against a basis of points of bn256's G1, on the device.
 *
 * halo2's prover commits to every column it builds: C_j = sum_i s_ji * P_i over the 2^k rows of column j, P_i the points of the
 * params' basis (the Lagrange basis for a column of values, the monomial one for coefficients: this library takes the points it
 * is given).  G1 is y^2 = x^3 + 3 over Fq, q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47, a group of
 * prime order r (cofactor 1).  One call commits n_cols columns against one basis by the bucket method with windows of one byte.
 *
 * A POINT is 64 bytes, 16-byte aligned: x then y, each eight little-endian 32-bit limbs of v * 2^256 mod q (Montgomery form).
 * The identity is 64 zero bytes (x = y = 0 is not on the curve).  aesw_msm_basis_device makes such points from the plain
 * little-endian coordinates a host reads from a params file, and checks them.  The commitments come out in the same form, so a
 * commitment can be a point of a later basis.  The compressed encoding of a transcript is the host's.
 *
 * SCALARS are either AESW_MSM_FR -- columns of Fr cells as every library of aesw.h writes them, [n_cols][2^k][32], eight
 * little-endian limbs of v * 2^256 mod r -- or AESW_MSM_BYTES -- columns of bytes, [n_cols][2^k], the value of a row its byte: what
 * the assembled advice columns of this circuit are.  A byte column is one window of the method and costs a thirty-second of a
 * column of cells.  16-byte aligned; n_cols * 2^k may pass 2^32 bytes: every offset is 64 bits.
 *
 * NON-CANONICAL CELLS (values at or above r) and basis points that are not on the curve: the commitments are unspecified; the
 * call still writes only its outputs and its workspace, and all of d_out.  There is no report on this call.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host and may be captured into a
 * hipGraph; the passes of a call are ordered by the stream, and the only atomics on memory are those of the basis call's report.
 * A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and the outputs untouched; aesw_last_error names the call and the
 * argument.  A group context is refused.  Bounds: 10 <= k <= 28, 1 <= n_cols <= 65535.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_msm -laesw. */
#ifndef AESW_MSM_H
#define AESW_MSM_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_MSM_FR 0u    /* d_scalars holds Fr cells, 32 bytes a row: 32 windows */
#define AESW_MSM_BYTES 1u /* d_scalars holds bytes, one a row: one window */

/* What aesw_msm_basis_device found: the points that are not on the curve or have a coordinate at or above q, and the index of
 * the first of them (~0: none). */
typedef struct aesw_msm_report {
    uint64_t bad_points;
    uint64_t first_bad;
} aesw_msm_report;

/* The rows of a chunk: what a workgroup sorts by digit at a time. */
uint32_t aesw_msm_chunk_rows(void);

/* The slices a call with these arguments cuts the rows into -- `slices` itself where it is not 0, else the rule's: about sixteen
 * workgroups a compute unit over (windows x columns), and no slice below two chunks; 0 outside the bounds.  Every slice but the
 * last is ceil(2^k / slices) rows rounded up to a multiple of 16. */
uint32_t aesw_msm_slices(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices);

/* Bytes of d_workspace for a call with these arguments: for cells 32 planes of 2^k bytes a column, then 256 accumulators of 96
 * bytes per slice, window and column, then one per window and column; 0 outside the bounds.  A multiple of 16.  Two calls in
 * flight need two. */
size_t aesw_msm_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices);

/* d_basis[i] = the point of the plain coordinates d_canonical[i], i < 2^k: [2^k][64], x then y, little-endian.  d_report counts
 * the points with a coordinate at or above q or with y^2 != x^3 + 3 and names the first; what is stored for such a point is of
 * no use.  d_basis may be d_canonical itself; a partial overlap is refused.  d_report: 8-byte aligned, reset by the call. */
int aesw_msm_basis_device(aesw_ctx *ctx, uint32_t k, const uint8_t *d_canonical, uint8_t *d_basis, aesw_msm_report *d_report, void *stream);

/* d_out[j] = sum_i d_scalars[j][i] * d_basis[i], j < n_cols: [n_cols][64].  scalars: AESW_MSM_FR or AESW_MSM_BYTES.  slices: 0 for
 * the rule's count, else 1 ... 2^k / 16 (at most 65535) -- the value changes the time and the workspace, never the result.
 * d_workspace: aesw_msm_workspace_bytes of the same arguments; it may not overlap anything else, nor d_out an input. */
int aesw_msm_commit_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices, const uint8_t *d_scalars, const uint8_t *d_basis,
                           uint8_t *d_out, void *d_workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_MSM_H */
