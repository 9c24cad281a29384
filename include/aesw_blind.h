/* aesw_blind.h -- C ABI of libaesw_blind.so: the blinding rows of a column, on the device, and the commitment of a column of bytes
 * whose last rows are blinded.
 *
 * A halo2 prover fills the last rows of every column it commits to with random cells, so that the openings of the proof say
 * nothing about the witness.  The device stages of this project write rows 0 ... n_rows - 1 and leave the rows from n_rows on to
 * the caller; this library writes them, where the columns lie, without a host round trip, so that the chain of stages stays one
 * sequence on a stream, and one graph.
 *
 * THE CELL is a pure function of (seed, domain, column, row):
 *   digest = BLAKE2b-512(key = seed[32], person = "aesw-blind-cells", message = le64(domain) || le64(column) || le64(row))
 *   cell   = the 64 bytes as a little-endian integer mod r, stored as an Fr cell in Montgomery form (eight little-endian 32-bit
 *            limbs of v * 2^256 mod r), canonical
 * which is Python's hashlib.blake2b(message, key=seed, person=b"aesw-blind-cells", digest_size=64), reduced.  The reduction of 64
 * bytes is what halo2curves' Fr::random does; its bias is below 2^-256.  `domain` is the caller's tag for a group of columns
 * (advice, A', S', Z, ...): groups filled under one seed share no cell.  THE SEED is 32 bytes of DEVICE memory, read when the
 * kernel runs: a captured graph follows a rewritten seed.  Draw it from the operating system; a proof is then reproducible from
 * its seed and no more predictable than it.  Which rows of which column a prover blinds is the caller's first_row.  Parity with
 * halo2's own random stream is not a goal.
 *
 * THE TAIL COMMITMENT.  An advice column of this circuit is bytes, and the library that commits columns takes it as one 8-bit window.  Blinded,
 * its last rows are cells; the commitment of the whole is the commitment of the bytes (with zero bytes in the tail rows) plus
 * sum_i tail[i] * P_i over the tail rows, which aesw_blind_commit_tail_device adds in place.  The scalars are secret: a term is a
 * fixed 254-step double-and-add in which the scalar's bit selects and never branches.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host and may be captured into a
 * hipGraph.  Offsets are 64-bit.  There is no atomic on memory.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and
 * everything untouched; aesw_last_error names the call and the argument.  A group context is refused.  Every pointer is 16-byte
 * aligned; an output may not overlap an input.  Bounds: 10 <= k <= 28, 1 <= n_cols <= 65535, first_row < 2^k, and for the
 * commitment 2^k - first_row <= AESW_BLIND_MAX_TAIL.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_blind -laesw. */
#ifndef AESW_BLIND_H
#define AESW_BLIND_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_BLIND_SEED_BYTES 32u
#define AESW_BLIND_MAX_TAIL 64u

/* The rules read back: the rows from first_row on, 2^k - first_row (0 outside the bounds above), and the most of them the
 * commitment takes, so that a test finds the edges without writing the numbers down. */
uint64_t aesw_blind_tail_rows(uint32_t k, uint64_t first_row);
uint32_t aesw_blind_max_tail(void);

/* Rows first_row ... 2^k - 1 of each of the n_cols columns of d_cells, [n_cols][2^k][32], and no other byte.  Column j is hashed as
 * column first_column + j.  first_row = 0 writes every row.  The stores follow the context's "fr_store_mode". */
int aesw_blind_rows_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, uint64_t domain, uint64_t first_column, const uint8_t *d_seed,
                           uint8_t *d_cells, void *stream);

/* The same cells, compactly: d_tail [n_cols][2^k - first_row][32].  For the columns whose body is bytes. */
int aesw_blind_tail_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, uint64_t domain, uint64_t first_column, const uint8_t *d_seed,
                           uint8_t *d_tail, void *stream);

/* d_commit[j] += sum_(i >= first_row) d_tail[j][i - first_row] * d_basis[i], in place: d_commit [n_cols][64] and d_basis [2^k][64] are
 * affine points as the commitments of this project lie in memory (x then y in Montgomery form, 64 zero bytes the identity), d_tail
 * [n_cols][2^k - first_row][32] any canonical cells -- they need not come from aesw_blind_tail_device.  2^k - first_row is at most
 * AESW_BLIND_MAX_TAIL.  A cell at or above r gives an unspecified point and in-bounds stores. */
int aesw_blind_commit_tail_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint64_t first_row, const uint8_t *d_tail, const uint8_t *d_basis, uint8_t *d_commit,
                                  void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_BLIND_H */
