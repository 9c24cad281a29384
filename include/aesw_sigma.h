/* aesw_sigma.h -- C ABI of libaesw_sigma.so: the grand products of halo2's PERMUTATION argument, on the device, from beta and gamma.
 *
 * The permutation argument enforces the copy_advice() equalities.  Its C columns of n = 2^k rows are cut into sets of
 * chunk_len columns (halo2: cs.degree() - 2); set s covers columns s * chunk_len ... min((s + 1) * chunk_len, C) - 1 and there are
 * S = ceil(C / chunk_len) sets.  Cell (c, i) has the label delta^c * omega^i, with omega = g^((r - 1) / 2^k), delta = g^(2^28)
 * and g = 7 the generator of bn256's scalar field.  For i < n_rows (the usable rows)
 *   num_s[i] = prod over c in set s of ( v_c[i] + beta * delta^c * omega^i  + gamma )
 *   den_s[i] = prod over c in set s of ( v_c[i] + beta * label(map[c][i])   + gamma )
 *   f_s[i]   = num_s[i] * inv(den_s[i]),  inv(0) = 0 (the convention of ff's batch_invert)
 *   Z_0[0] = 1,   Z_s[i + 1] = Z_s[i] * f_s[i],   Z_(s+1)[0] = Z_s[n_rows]
 * and the argument holds exactly when Z_(S-1)[n_rows] = 1.  This restates plonk/permutation/prover.rs::commit of halo2_proofs
 * v0.3.0 (the PSE fork); parity with halo2's own keygen mapping is not pinned by a test.
 *
 * SIGMA IS A COLUMN OF CELL INDICES: map[c][i] = c' * 2^k + i', one uint32_t per cell (C * 2^k <= 2^32), not a 32-byte label.
 * A VALUE v_c[i] IS A BYTE: every cell of this circuit's advice columns and of its fixed round_constants column is one.
 * AN Fr CELL is 32 bytes: eight little-endian 32-bit limbs of v * 2^256 mod r -- the Montgomery form of every Fr cell of aesw.h.
 *
 * THE COLUMNS OF A FixedAes128Config<k, n_sets> CIRCUIT, in the order configure() enables equality on them:
 *   x0 y0 z0 words_column round_constants x1 y1 z1 x2 ...          C = 3 * n_sets + 2
 * (src/key_schedule.rs:52-57 runs before the loop of src/aes128.rs:126-130).  round_constants is a FIXED column; it takes part in
 * no copy, so its sigma is the identity, but it shifts the delta exponent of every column behind it.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host, writes every output word
 * itself with plain stores -- no atomic, nothing to reset -- and may be captured into a hipGraph: a replay rebuilds its outputs
 * and its report from what beta, gamma and the columns then hold.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued
 * and the outputs untouched; aesw_last_error names the call.  A group context is refused.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with -laesw_sigma -laesw. */
#ifndef AESW_SIGMA_H
#define AESW_SIGMA_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aesw_sigma_report {
    uint64_t sets;         /* S = ceil(n_cols / chunk_len) */
    uint64_t open;         /* 1: the last closing product is not 1 */
    uint64_t zero_terms;   /* rows of sets whose den is zero (0 when noncanonical) */
    uint64_t first_zero;   /* AESW_CHECK_NONE, or the smallest set * 2^k + row among them */
    uint64_t out_of_range; /* entries of d_map at or above n_cols * 2^k (each read as the cell itself) in the rows below n_rows,
                              plus entries of d_source at or above n_advice + n_fixed (such a column reads as zero bytes) */
    uint64_t noncanonical; /* 1: beta >= r or gamma >= r; every written cell of Z and of the closing cells is zero */
} aesw_sigma_report;

/* ---- pure host: no device, no context ---- */

/* 3 * n_sets + 2 */
uint32_t aesw_sigma_columns(uint32_t n_sets);

/* source[c] for the 3 * n_sets + 2 permutation columns in halo2's order: below 3 * n_sets + 1 that assembled advice column
 * (aesw_assemble_advice_device's order), 3 * n_sets + 1 the fixed round_constants column -- d_source of the product call with
 * n_advice = 3 * n_sets + 1 and n_fixed = 1.  n_sets 1 ... 1024. */
int aesw_sigma_sources_host(uint32_t n_sets, uint32_t *source);

/* The mapping of a FixedAes128Config<k, n_sets> circuit with one schedule_key and n_blocks encrypt calls:
 * map[3 * n_sets + 2][2^k] uint32_t.  halo2's permutation::keygen::Assembly restated: the identity, then copy(left, right) for
 * every copy_advice() in synthesize()'s call order (aesw_key_copy_graph, then aesw_block_copy_graph per block placed by
 * aesw_block_placement; left is the new cell, right the copied one): nothing if both lie in one cycle; else the larger cycle
 * is "left" (on equal sizes the call's left), the smaller one is relabelled, and mapping[left] and mapping[right] swap.
 * AESW_ERR_CAPACITY when n_blocks is above aesw_block_capacity(k, n_sets); AESW_ERR_INVALID_ARG for k outside 10 ... 28,
 * n_sets outside 1 ... 1024 or (3 * n_sets + 2) * 2^k above 2^32. */
int aesw_sigma_mapping_host(uint32_t k, uint32_t n_sets, uint32_t n_blocks, uint32_t *map);

/* Bytes of d_tables and of d_workspace; 0 outside the bounds of the calls below.  Multiples of 16. */
size_t aesw_sigma_tables_bytes(uint32_t k, uint32_t n_cols);
size_t aesw_sigma_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t chunk_len);

/* ---- device ---- */

/* The power tables, challenge free, once per (k, n_cols): d_tables (16-byte aligned, aesw_sigma_tables_bytes) holds
 *   omega^j for j < 2^min(k, 14),  then omega^(j * 2^14) for j < 2^max(k - 14, 0),  then delta^c for c < n_cols
 * so omega^i is low[i & 16383] * high[i >> 14].  k 10 ... 28 (the field's 2-adicity is 28), n_cols 1 ... 3074,
 * n_cols * 2^k <= 2^32. */
int aesw_sigma_tables_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint8_t *d_tables, void *stream);

/* Z of the S sets.
 *   d_advice      [n_advice][2^k] bytes, d_fixed [n_fixed][2^k] bytes, 16-byte aligned; either may be NULL when its count is 0
 *   d_source      [n_cols]: an entry below n_advice selects an advice column, one from n_advice up to n_advice + n_fixed - 1 a
 *                 fixed column; any other is counted in out_of_range and its column reads as zero bytes
 *   d_map         [n_cols][2^k] cell indices, 16-byte aligned; rows 0 ... n_rows - 1 are used (read four at a time, so up to
 *                 three rows behind n_rows are read and ignored)
 *   d_tables      what aesw_sigma_tables_device wrote for the same (k, n_cols)
 *   d_beta, d_gamma  one Fr cell each in device memory, 16-byte aligned, read when the kernels run
 *   d_z_fr        [S][2^k][32], 16-byte aligned: rows 0 ... min(n_rows, 2^k - 1) of every set are written, each word once; the
 *                 rows above are the caller's blinding rows and are not written.  Stores follow the context's "fr_store_mode".
 *   d_closing_fr  [S][32], 16-byte aligned: Z_s[n_rows], always written
 *   d_workspace   aesw_sigma_workspace_bytes(k, n_cols, chunk_len) bytes, 16-byte aligned; two calls in flight need two
 *   d_report      8-byte aligned; set by the call
 * k 10 ... 28, n_cols 1 ... 3074, n_cols * 2^k <= 2^32, chunk_len 1 ... 8, 1 <= n_rows <= 2^k.
 * A zero term (den = 0) makes Z zero behind its row, in its set and in every later one. */
int aesw_sigma_product_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t chunk_len, uint32_t n_rows,
                              const uint8_t *d_advice, uint32_t n_advice, const uint8_t *d_fixed, uint32_t n_fixed,
                              const uint32_t *d_source, const uint32_t *d_map, const uint8_t *d_tables, const uint8_t *d_beta,
                              const uint8_t *d_gamma, uint8_t *d_z_fr, uint8_t *d_closing_fr, void *d_workspace,
                              aesw_sigma_report *d_report, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_SIGMA_H */
