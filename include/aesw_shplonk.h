/* aesw_shplonk.h -- C ABI of libaesw_shplonk.so: SHPLONK's multi-opening argument over coefficient columns, on the device: every
 * queried column opened at its points in two quotients, h and W.
 *
 * The rule is halo2_proofs v0.3.0 poly/kzg/multiopen/shplonk/prover.rs restated from memory.  Parity with halo2 is NOT PINNED by
 * a test here.  One difference is known: halo2 orders the point sets by the value of their points, which needs x on the
 * host; here the order of the sets, and of the columns within a set, is the caller's.
 *
 * A PLAN is static and made on the host.  It holds n_points distinct super-set points (d_points, cells in device memory,
 * 1 ... 16 of them) and n_sets sets (1 ... 16).  Set i has set_points[i] = t_i strictly increasing indices into the super set
 * (1 ... 8; point_index holds them one set behind the other) and set_cols[i] = m_i columns (1 ... 65535).  The plan crosses the ABI as
 * plain host arrays, read and checked before anything is enqueued; the prepare call lays it at the front of the scalars block,
 * where the later calls read it when their kernels run.
 *
 * With y, v, u cells in device memory and e_ijs the evaluation of column j of set i at the set's point s:
 *   N^P_i(X) = sum_j y^j P_ij(X)                 e_is = sum_j y^j e_ijs
 *   R_i(X)   the interpolant through (z_s, e_is); N_i = N^P_i - R_i differs from N^P_i in its low t_i cells
 *   Q_i      = N_i / prod_s (X - z_s) = sum_s w_is kate(N_i, z_s),  w_is = 1 / prod_(r != s) (z_s - z_r)
 *   h(X)     = sum_i v^i Q_i(X)                  commit, write_point, squeeze u
 *   z_i      = prod_(p not in set i) (u - p),  z_T = prod_p (u - p)
 *   L(X)     = sum_i v^i z_i (N^P_i(X) - R_i(u)) - z_T h(X)
 *   W(X)     = z_0^-1 L(X) / (X - u), remainder 0: the divide call of the library that evaluates, folds and
 *            divides coefficient columns, at u on L' = z_0^-1 L; no division kernel of this library's own.  Commit, write_point.
 * Transcript order: squeeze y, squeeze v, write [h], squeeze u, write [W].
 *
 * CELLS are those of every Fr library here: eight little-endian 32-bit limbs of v * 2^256 mod r, 16-byte aligned; a COLUMN is 2^k of them.
 * NON-CANONICAL input cells give unspecified values and in-bounds stores.
 *
 * THE SCALARS BLOCK (aesw_shplonk_scalars_bytes) holds every small table; aesw_shplonk_scalars_offset gives the byte offset of each,
 * so a caller never hard-codes the layout.  THE REPORT is eight 64-bit words, 16-byte aligned:
 *   0  sets with a remainder N_i(z_s) that is not 0 -- the evaluations do not belong to the columns; the quotient written is still
 *      the partial-fraction sum
 *   1  the lowest such set, or ~0
 *   2  point differences z_s - z_r of a set that are 0 (two equal points in a set: their weight is taken as 0)
 *   3  1 where z_0 = 0
 *   4 ... 7  the remainder of the last division as a cell: pass d_report + AESW_SHPLONK_REPORT_LAST_REM as d_rem of
 *      that divide call.  The prepare call zeroes it.
 * The prepare call resets the report; the quotient calls add to words 0 and 1 in stream order; the finish call sets word 3.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, uses no atomic and may be
 * captured into a hipGraph.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and aesw_last_error set.  A group
 * context is refused.  10 <= k <= 28; every offset is 64 bits.
 *
 * The library links against libaesw.so alone ($ORIGIN).  Link with -laesw_shplonk -laesw. */
#ifndef AESW_SHPLONK_H
#define AESW_SHPLONK_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_SHPLONK_REPORT_LAST_REM 32u /* the byte offset of report words 4 ... 7 */

/* the tables of the scalars block, for aesw_shplonk_scalars_offset */
#define AESW_SHPLONK_PLAN 0u    /* the plan, 1 024 bytes */
#define AESW_SHPLONK_V_POW 1u   /* [16]     v^i */
#define AESW_SHPLONK_EBAR 2u    /* [16][8]  e_is */
#define AESW_SHPLONK_W 3u       /* [16][8]  w_is */
#define AESW_SHPLONK_VW 4u      /* [16][8]  v^i w_is */
#define AESW_SHPLONK_NEG_R 5u   /* [16][8]  the t_i coefficients of -R_i from the constant up: d_low of the combine that makes N_i */
#define AESW_SHPLONK_Z 6u       /* [16]     z_i */
#define AESW_SHPLONK_Z_T 7u     /*          z_T */
#define AESW_SHPLONK_Z0_INV 8u  /*          z_0^-1 */
#define AESW_SHPLONK_L_COEF 9u  /* [S + 1]  z_0^-1 v^i z_i for set i, then -z_0^-1 z_T for h: d_coefs of the combine that makes L' */
#define AESW_SHPLONK_L_CONST 10u /*         -z_0^-1 sum_i v^i z_i R_i(u): d_low (n_low = 1) of that combine over the columns N^P_i and h */
#define AESW_SHPLONK_L_LOW 11u  /* [8]      the same with z_0^-1 sum_i v^i z_i R_i(X) added: d_low (n_low = 8) of that combine over the columns N_i and h */
#define AESW_SHPLONK_Y_POW 12u  /* [max m]  y^j: d_coefs of the combine that makes N_i */

/* Bytes of d_scalars for a plan of n_sets sets whose largest has max_cols columns; 0 outside the bounds.  A multiple of 16. */
size_t aesw_shplonk_scalars_bytes(uint32_t n_sets, uint32_t max_cols);
/* The byte offset in d_scalars of the cells of `table` that belong to set `set` (0 for a table that has one entry; n_sets for the
 * entry of h in AESW_SHPLONK_L_COEF); (size_t)-1 for a table or a set there is none of. */
size_t aesw_shplonk_scalars_offset(uint32_t table, uint32_t set);
/* Bytes of d_workspace of a quotient call at k, whatever the set; 0 outside the bounds.  A multiple of 16. */
size_t aesw_shplonk_workspace_bytes(uint32_t k);
/* Bytes of d_report: 64. */
size_t aesw_shplonk_report_bytes(void);

/* The small phase after y and v: writes the plan, y^j, v^i, e_is, w_is, v^i w_is and -R_i into d_scalars and resets d_report.
 * d_points [n_points][32]; d_evals [sum m_i t_i][32], set by set, column by column, point by point; d_y, d_v one cell each. */
int aesw_shplonk_prepare_device(aesw_ctx *ctx, uint32_t n_points, uint32_t n_sets, const uint32_t *set_points, const uint32_t *set_cols,
                                const uint32_t *point_index, const uint8_t *d_points, const uint8_t *d_evals, const uint8_t *d_y, const uint8_t *d_v,
                                uint8_t *d_scalars, void *d_report, void *stream);

/* The small phase after u: writes z_i, z_T, z_0^-1, the S + 1 coefficients of L' = z_0^-1 L, its constant and its low cells into
 * the d_scalars a prepare call wrote, whose plan it reads, and sets report word 3. */
int aesw_shplonk_finish_device(aesw_ctx *ctx, const uint8_t *d_points, const uint8_t *d_u, uint8_t *d_scalars, void *d_report, void *stream);

/* d_out[r] = acc[r] + sum_j d_coefs[j] * col_j[r], r < 2^k, plus d_low[r] for r < n_low <= 8.  d_coeff [n_cols][2^k][32], d_coefs
 * [n_cols][32] read when the kernel runs (usually a slice of the scalars block), d_low [n_low][32] or NULL with n_low = 0, acc is
 * d_acc_in [2^k][32] or zero where it is NULL; d_acc_in == d_out is allowed, so columns in separate allocations take successive
 * calls.  One call serves N_i (coefficients y^j, low cells -R_i) and L'.  Stores follow the context's "fr_store_mode". */
int aesw_shplonk_combine_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_coeff, const uint8_t *d_coefs, const uint8_t *d_low,
                                uint32_t n_low, const uint8_t *d_acc_in, uint8_t *d_out, void *stream);

/* d_out = acc + v^i Q_i for set i = `set` of the plan in d_scalars, Q_i the partial-fraction sum over the set's points of the
 * quotients of d_numer = N_i, in three passes over the numerator.  d_rem [8][32]: cell s < t_i becomes N_i(z_s), the others are
 * left alone.  d_out == d_acc_in is allowed (h accumulates over the sets) and so is d_out == d_numer; any other overlap is
 * refused.  d_workspace aesw_shplonk_workspace_bytes(k).  Adds the set to report words 0 and 1 where a remainder is not 0.
 * Stores of d_out follow the context's "fr_store_mode". */
int aesw_shplonk_quotient_device(aesw_ctx *ctx, uint32_t k, uint32_t set, const uint8_t *d_numer, const uint8_t *d_points, const uint8_t *d_scalars,
                                 const uint8_t *d_acc_in, uint8_t *d_out, uint8_t *d_rem, void *d_workspace, void *d_report, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_SHPLONK_H */
