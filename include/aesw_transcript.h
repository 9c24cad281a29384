/* aesw_transcript.h -- C ABI of libaesw_transcript.so: the Blake2b transcript of a halo2 prover, on the device.
 *
 * halo2's prover derives every challenge from a hash of what it has committed to so far and writes the same values into the
 * proof: Blake2bWrite<_, G1Affine, Challenge255<_>>.  With the commitments and the evaluations in device memory and every
 * prover-side call reading its challenges from device memory, this library is the link between the two: points and scalars are
 * absorbed where they lie, a challenge is squeezed into a 32-byte cell on the device, and the proof bytes are appended to a
 * device buffer.  No call waits on the host, so the device stages of a proof are one sequence on a stream, and one graph.
 *
 * THE RULE (halo2_proofs v0.3.0 transcript.rs, halo2curves 0.3.3 bn256::G1Affine::to_bytes, restated from memory:
 * parity with halo2 NOT PINNED; what is pinned is Blake2b itself, against Python's hashlib):
 *   the hash     Blake2b-512, no key, no salt, person "Halo2-Transcript";
 *   a point      absorbed as the byte 0x01, then x and y as 32 little-endian bytes of the plain value each (65 bytes); written to
 *                the proof as x's 32 plain bytes with (y & 1) << 7 OR-ed into byte 31;
 *   a scalar     absorbed as 0x02 and its 32 little-endian plain bytes (33 bytes); written as those 32 bytes;
 *   a challenge  the byte 0x00 is absorbed, a COPY of the hash is finalised to 64 bytes and the live hash goes on; the challenge
 *                is the 64 bytes as a little-endian integer mod r, stored as an Fr cell in Montgomery form;
 *   item i of a call is absorbed after item i - 1: a call with n items is n calls of halo2's method.
 * THE IDENTITY.  A POINT is 64 bytes, x then y, each eight little-endian 32-bit limbs of v * 2^256 mod q, as the commitments of
 * this project lie in memory; 64 zero bytes are the identity, which halo2 refuses to write.  Here it is counted in the state's
 * report words, absorbed as 0x01 and 64 zero bytes and written as 32 zero bytes: deterministic, in bounds, and the caller reads
 * the count.  A CELL is 32 bytes, eight little-endian limbs of v * 2^256 mod r.  Coordinates and cells at or above their modulus
 * are taken out of Montgomery form like any other: the result is some value below the modulus, and every store stays in bounds.
 *
 * THE STATE is AESW_TRANSCRIPT_STATE_BYTES of device memory, 16-byte aligned, thirty-two little-endian 64-bit words:
 *   words 0 ... 7   the chain value h of Blake2b
 *   word 8          the bytes compressed so far
 *   words 9 ... 24  the block: up to 128 bytes not yet compressed (Blake2b keeps a full last block until more input arrives or
 *                   the hash is finalised); the bytes from `fill` on are zero
 *   word 25         fill, 0 ... 128
 *   word 26         proof bytes produced: the proof's cursor -- a call appends at d_proof + this, so a replayed graph appends where
 *                   the last call stopped
 *   word 27         proof bytes that did not fit: the bytes at or past proof_capacity are not stored but counted here
 *   word 28         identity points seen
 *   word 29         the index of the first of them among the points absorbed since init (~0: none)
 *   word 30         points absorbed since init
 *   word 31         0
 * aesw_transcript_init_device writes all of it.  A call on a state nobody initialised hashes nonsense and stays in bounds.
 *
 * Every device call is asynchronous on `stream`, allocates nothing, waits for nothing on the host and may be captured into a
 * hipGraph.  A call is one workgroup: a transcript is serial, and what counts is its latency.  There is no atomic on memory.
 * Calls on one state are ordered by the stream.  A refusal returns AESW_ERR_INVALID_ARG with nothing enqueued and everything
 * untouched; aesw_last_error names the call and the argument.  A group context is refused.  Every pointer is 16-byte aligned; the
 * state, the items, the proof and the challenge of a call may not overlap.  Bounds: 1 <= n <= 65535.
 *
 * The library links against libaesw.so alone ($ORIGIN) and takes the aesw_ctx that aesw_create made.  Link with
 * -laesw_transcript -laesw. */
#ifndef AESW_TRANSCRIPT_H
#define AESW_TRANSCRIPT_H

#include <stddef.h>

#include "aesw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AESW_TRANSCRIPT_STATE_BYTES 256u

/* The items a call lays into on-chip memory at a time: a test reaches a second chunk by passing more. */
uint32_t aesw_transcript_chunk_points(void);
uint32_t aesw_transcript_chunk_scalars(void);

/* A fresh transcript: nothing absorbed, the cursor at 0, no identity seen. */
int aesw_transcript_init_device(aesw_ctx *ctx, uint8_t *d_state, void *stream);

/* n points, d_points [n][64], absorbed in order.  d_proof == NULL and proof_capacity == 0: common_point.  Otherwise write_point:
 * the 32 compressed bytes of each are also appended at the state's cursor, and of those the bytes at or past proof_capacity are
 * counted, not stored; absorption is unaffected.  One of the two without the other is refused. */
int aesw_transcript_points_device(aesw_ctx *ctx, uint8_t *d_state, uint32_t n, const uint8_t *d_points, uint8_t *d_proof, uint64_t proof_capacity, void *stream);

/* n scalars, d_cells [n][32] Fr cells in Montgomery form: common_scalar, or with d_proof write_scalar (32 plain bytes each). */
int aesw_transcript_scalars_device(aesw_ctx *ctx, uint8_t *d_state, uint32_t n, const uint8_t *d_cells, uint8_t *d_proof, uint64_t proof_capacity, void *stream);

/* squeeze_challenge: d_challenge [32], one Fr cell in Montgomery form -- what every call that reads a challenge from device memory
 * takes. */
int aesw_transcript_squeeze_device(aesw_ctx *ctx, uint8_t *d_state, uint8_t *d_challenge, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AESW_TRANSCRIPT_H */
