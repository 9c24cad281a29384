/* aesw_vanish.h -- C ABI of libaesw_vanish.so: the vanishing argument's quotient h(X) of a FixedAes128Config<k, n_sets> circuit
 * on the extended coset, halo2's evaluate_h, folded on the device one constraint segment per call.
 *
 * n = 2^k, E = 2^ext_k, m = E / n.  Row j of an extended column is the column's polynomial at x_j = zeta * omega_ext^j.  The
 * numerator folds the circuit's constraints with  acc = acc * y + constraint,  which is linear in acc: a SEGMENT of `len`
 * consecutive constraints is  acc_out[j] = acc_in[j] * y^len + seg(j),  seg the same fold started from 0, and the calls of the
 * segments in their order are the whole fold:
 *   HEAD        the gate  q_rcon * (words - rcon);  l0 * (1 - Zp_0);  l_last * (Zp_(S-1)^2 - Zp_(S-1));
 *               for s = 1 ... S-1: l0 * (Zp_s - Zp_(s-1)[rot n_rows]).  len = S + 2.  It opens the fold: there is no acc_in.
 *   PERM(s)     s = 0 ... S-1:  l_active * (Zp_s[rot 1] * prod_c (v_c + beta * sigma_c + gamma)
 *                                           - Zp_s * prod_c (v_c + beta * delta^c * x_j + gamma)),  c over set s.  len = 1.
 *   LOOKUP(s)   s = 0 ... n_sets-1, for tag t = 1 ... 5:  l0 * (1 - Z);  l_last * (Z^2 - Z);
 *               l_active * (Z[rot 1] * (A' + beta) * (S' + gamma) - Z * (in + beta) * (tab + gamma));  l0 * (A' - S');
 *               l_active * (A' - S') * (A' - A'[rot -1]),  in and tab the set's columns and the table compressed under theta.  len = 25.
 *   DIVIDE      acc * inv(x_j^n - 1), the output.
 * S = ceil((3 n_sets + 2) / chunk_len) permutation sets.  A rotation by r rows of the circuit reads row (j + r * m) mod E.
 * A segment reads only its own columns, so a caller need not hold every extended column at once: it extends a group, folds it,
 * and uses the buffer again.
 *
 * The rule is plonk/evaluation.rs of halo2_proofs v0.3.0 restated from memory.  NOT PINNED against halo2 by a test here: the
 * order of the constraints, and zeta (zeta_sel 0: g^((r - 1) / 3), 1: its square).
 *
 * CELLS are those of every Fr library here: eight little-endian 32-bit limbs of v * 2^256 mod r, 16-byte aligned.  Each group
 * pointer is a contiguous [columns][2^ext_k][32], so a slice of a larger tensor serves.  NON-CANONICAL input cells give
 * unspecified values and in-bounds stores.
 *
 * THE TABLES (aesw_vanish_tables_bytes) are free of the challenges: inv(x^n - 1) for the m values of x^n, and the powers x_j is
 * one product of.  THE SCALARS BLOCK (aesw_vanish_scalars_bytes) holds everything a segment needs that is per proof and not per
 * row; a small kernel derives it from theta, beta, gamma and y, cells in device memory read when it runs, so a captured graph
 * follows new challenges.  aesw_vanish_scalars_offset gives the byte offset of each entry, so a caller never hard-codes the layout.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, uses no atomic and may be
 * captured into a hipGraph.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and aesw_last_error set.  A group
 * context is refused.  Bounds: 10 <= k, ext_k <= 28, 2 <= ext_k - k, zeta_sel <= 1, 1 <= n_sets <= 1024, 1 <= chunk_len <= 8 and
 * chunk_len + 2 <= m + 1, 1 <= n_rows < 2^k.  Every offset is 64 bits.  d_acc_in == d_acc_out is allowed; any other overlap
 * of an output with an input is refused.  Stores of d_acc_out follow the context's "fr_store_mode".
 *
 * The library links against libaesw.so alone ($ORIGIN).  Link with -laesw_vanish -laesw. */
#ifndef AESW_VANISH_H
#define AESW_VANISH_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the entries of the scalars block, for aesw_vanish_scalars_offset */
#define AESW_VANISH_THETA 0u      /*        theta, as it was when the scalars call ran */
#define AESW_VANISH_BETA 1u       /*        beta */
#define AESW_VANISH_GAMMA 2u      /*        gamma */
#define AESW_VANISH_Y 3u          /*        y */
#define AESW_VANISH_Y_POW 4u      /* [3]    y^len of HEAD, PERM and LOOKUP */
#define AESW_VANISH_THETA_POW 5u  /* [2]    theta^2, theta^3 */
#define AESW_VANISH_TAG 6u        /* [5]    t * theta^(arity(t) - 1) for tag t = 1 ... 5 */
#define AESW_VANISH_DELTA 7u      /* [S]    delta^first(s), first(s) = s * chunk_len; 64 bytes apart */
#define AESW_VANISH_BETA_DELTA 8u /* [S]    beta * delta^first(s); 64 bytes apart */

/* 1 where the shape is within the bounds above, which every segment call holds (zeta_sel only where it is an argument), else 0. */
int aesw_vanish_shape_ok(uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows);

/* Bytes of d_tables; 0 outside the bounds.  A multiple of 32. */
size_t aesw_vanish_tables_bytes(uint32_t k, uint32_t ext_k);
/* Writes the tables of (k, ext_k, zeta_sel) into d_tables. */
int aesw_vanish_tables_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint8_t *d_tables, void *stream);

/* Bytes of d_scalars; 0 outside the bounds.  A multiple of 32. */
size_t aesw_vanish_scalars_bytes(uint32_t n_sets, uint32_t chunk_len);
/* The byte offset in d_scalars of entry `index` of `table`; (size_t)-1 for a table or an entry there is none of. */
size_t aesw_vanish_scalars_offset(uint32_t table, uint32_t index);
/* Derives the scalars block from the four challenges, one cell each in device memory. */
int aesw_vanish_scalars_device(aesw_ctx *ctx, uint32_t n_sets, uint32_t chunk_len, const uint8_t *d_theta, const uint8_t *d_beta, const uint8_t *d_gamma,
                               const uint8_t *d_y, uint8_t *d_scalars, void *stream);

/* HEAD.  d_words [1]: the round-constant advice column (the last advice column); d_rcon [2]: the fixed round constants, then
 * their selector; d_zperm [S]: the permutation's grand products; d_l [3]: l0, l_last, l_active.  Writes d_acc_out [2^ext_k][32]. */
int aesw_vanish_head_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, const uint8_t *d_words,
                            const uint8_t *d_rcon, const uint8_t *d_zperm, const uint8_t *d_l, const uint8_t *d_scalars, uint8_t *d_acc_out, void *stream);

/* PERM(set).  d_values and d_sigma hold only the columns of that set, in the permutation's order (x0 y0 z0 words rcon x1 y1 z1
 * ...): end(set) - first(set) columns each; d_z [1]: Zp_set; d_l [3]. */
int aesw_vanish_perm_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, uint32_t set, const uint8_t *d_values,
                            const uint8_t *d_sigma, const uint8_t *d_z, const uint8_t *d_l, const uint8_t *d_tables, const uint8_t *d_scalars, const uint8_t *d_acc_in,
                            uint8_t *d_acc_out, void *stream);

/* LOOKUP(set).  d_advice3 [3]: the set's advice columns x, y, z; d_selectors5, d_a5, d_s5, d_z5 [5]: the selector, the permuted
 * input A', the permuted table S' and the grand product Z of the set's five arguments, tag 1 first; d_table4 [4]: the table; d_l [3]. */
int aesw_vanish_lookup_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t n_sets, uint32_t chunk_len, uint32_t n_rows, uint32_t set, const uint8_t *d_advice3,
                              const uint8_t *d_selectors5, const uint8_t *d_table4, const uint8_t *d_a5, const uint8_t *d_s5, const uint8_t *d_z5, const uint8_t *d_l,
                              const uint8_t *d_scalars, const uint8_t *d_acc_in, uint8_t *d_acc_out, void *stream);

/* DIVIDE: d_acc_out[j] = d_acc_in[j] * inv(x_j^n - 1). */
int aesw_vanish_divide_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, const uint8_t *d_tables, const uint8_t *d_acc_in, uint8_t *d_acc_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_VANISH_H */
