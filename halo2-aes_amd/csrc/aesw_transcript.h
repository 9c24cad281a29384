// aesw_transcript.h -- the rules of libaesw_transcript.so, once: the Blake2b transcript a halo2 prover derives its
// challenges from and writes its proof through, Blake2bWrite<_, G1Affine, Challenge255<_>>, for the kernels of
// transcript/aesw_transcript.hip and for the CPU driver of tests/transcript_driver.cpp.  The fields are aesw_fq.h's (coordinates) and
// aesw_fr.h's (scalars, challenges); nothing of either is restated.  No HIP call and no ROCm include: tests/test_transcript_model.py
// compiles this header alone with g++.
//
// THE RULE is the behaviour of halo2_proofs v0.3.0 transcript.rs and of halo2curves 0.3.3 bn256::G1Affine::to_bytes, restated from
// memory: parity with halo2 NOT PINNED.  What is pinned, exactly, is Python's hashlib.blake2b, which implements the same function
// (tests/transcript_model.py).
// STATE.  A streaming Blake2b-512: digest_size 64, no key, no salt, person "Halo2-Transcript".  Blake2b compresses a full block only
// once more input arrives (the last block is compressed with the final flag, and a message of exactly 128 bytes has one block): the
// state keeps up to 128 bytes, `fill` of them, and `count` the bytes already compressed.
// common_point(P): the byte 0x01, then x and y as 32 little-endian bytes of the plain value each (out of Montgomery form): 65 bytes.
// common_scalar(s): 0x02, then the 32 little-endian plain bytes: 33 bytes.
// squeeze_challenge(): 0x00 is absorbed, a COPY of the state is finalised to 64 bytes, the live state goes on (with the 0x00).  The
// challenge is the 64 bytes as a little-endian integer mod r, as a Montgomery cell (fr_from_u512).
// write_point(P): common_point(P), then 32 bytes to the proof -- x's plain little-endian bytes with (y & 1) << 7 OR-ed into byte 31.
// write_scalar(s): common_scalar(s), then the 32 plain bytes.
// THE IDENTITY (x = y = 0, the affine identity of aesw_msm.h) is an error in halo2.  Here it is counted (the report words), absorbed
// as 0x01 and 64 zero bytes and written as 32 zero bytes, which is what the rule above gives for x = y = 0 anyway.
//
// fr_from_u512: lo + hi * 2^256 mod r in Montgomery form is mont_mul(lo, R^2) + mont_mul(hi, R^3), lo and hi the 256-bit halves,
// either of which may be at or above r.  The one CIOS product of aesw_mont.h still returns a canonical value for a < 2^256 against
// b < r: with R = 2^256 the value before the last subtraction is (a b + k r) / R with k < R, below (R r + R r) / R = 2 r, so
// mont_reduce_once's single subtraction ends below r; and on the way the running value after i + 1 limbs of b is below a + r <
// 2^256 + 2^254, which the ninth limb the loop carries (t[MONT_LIMBS]) holds.  The static_assert below evaluates both halves at
// 2^256 - 1.
#pragma once
#include <stdint.h>

#include "aesw_fq.h"
#include "aesw_fr.h"

namespace aesw {

constexpr uint32_t TRANSCRIPT_STATE_BYTES = 256, TRANSCRIPT_BLOCK = 128, TRANSCRIPT_DIGEST = 64;
constexpr uint32_t TRANSCRIPT_POINT_MESSAGE = 65, TRANSCRIPT_SCALAR_MESSAGE = 33, TRANSCRIPT_PROOF_ITEM = 32;
constexpr uint32_t TRANSCRIPT_MAX_ITEMS = 65535;
constexpr uint8_t TRANSCRIPT_TAG_CHALLENGE = 0, TRANSCRIPT_TAG_POINT = 1, TRANSCRIPT_TAG_SCALAR = 2;
// what a workgroup lays into LDS at a time: a lane per coordinate or per cell
constexpr uint32_t TRANSCRIPT_LANES = 64, TRANSCRIPT_CHUNK_POINTS = TRANSCRIPT_LANES / 2, TRANSCRIPT_CHUNK_SCALARS = TRANSCRIPT_LANES;
constexpr uint32_t TRANSCRIPT_CHUNK_BYTES = TRANSCRIPT_CHUNK_SCALARS * TRANSCRIPT_SCALAR_MESSAGE;
static_assert(TRANSCRIPT_CHUNK_POINTS * TRANSCRIPT_POINT_MESSAGE <= TRANSCRIPT_CHUNK_BYTES, "a chunk of scalars is the longer one");
// the stream of a chunk: the bytes the state kept, the chunk's messages behind them, and the block the remainder is read from
constexpr uint32_t TRANSCRIPT_STREAM_WORDS = (TRANSCRIPT_BLOCK + TRANSCRIPT_CHUNK_BYTES + TRANSCRIPT_BLOCK + 7) / 8;

constexpr bool transcript_items_ok(uint32_t n) { return n >= 1 && n <= TRANSCRIPT_MAX_ITEMS; }

// The state as it lies in memory, 256 bytes of little-endian 64-bit words: h[8], the bytes compressed, the block (byte i of it is
// byte i % 8 of word i / 8; the bytes from `fill` on are zero), fill, then the report words -- the proof bytes produced (the
// cursor: a call appends there), those of them that did not fit, the identity points seen, the index of the first among the points
// absorbed since init (~0: none) -- and the points absorbed.
struct TranscriptState {
    uint64_t h[8];
    uint64_t count;
    uint64_t block[16];
    uint64_t fill;
    uint64_t proof_bytes, proof_missed, identities, first_identity;
    uint64_t points;
    uint64_t reserved;
};
static_assert(sizeof(TranscriptState) == TRANSCRIPT_STATE_BYTES, "the state is 256 bytes");

// ---- Blake2b ----------------------------------------------------------------------------------------------------------------------
constexpr uint64_t BLAKE2B_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                    0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
// the parameter block: digest length 64, key length 0, fanout 1, depth 1 in word 0; the 16 bytes of the person in words 6 and 7
constexpr uint64_t BLAKE2B_PARAM0 = 0x01010040ull, TRANSCRIPT_PERSON0 = 0x72542d326f6c6148ull /* "Halo2-Tr" */, TRANSCRIPT_PERSON1 = 0x7470697263736e61ull /* "anscript" */;

AESW_MONT_HD constexpr uint64_t blake2b_rotr(uint64_t v, int n) { return (v >> n) | (v << (64 - n)); }

#define AESW_B2B_G(a, b, c, d, x, y)         \
    v[a] += v[b] + (x);                      \
    v[d] = blake2b_rotr(v[d] ^ v[a], 32);    \
    v[c] += v[d];                            \
    v[b] = blake2b_rotr(v[b] ^ v[c], 24);    \
    v[a] += v[b] + (y);                      \
    v[d] = blake2b_rotr(v[d] ^ v[a], 16);    \
    v[c] += v[d];                            \
    v[b] = blake2b_rotr(v[b] ^ v[c], 63);
// a round under one row of sigma: every index of w is a constant, so the sixteen words stay in registers
#define AESW_B2B_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    AESW_B2B_G(0, 4, 8, 12, w[s0], w[s1])                                                    \
    AESW_B2B_G(1, 5, 9, 13, w[s2], w[s3])                                                    \
    AESW_B2B_G(2, 6, 10, 14, w[s4], w[s5])                                                   \
    AESW_B2B_G(3, 7, 11, 15, w[s6], w[s7])                                                   \
    AESW_B2B_G(0, 5, 10, 15, w[s8], w[s9])                                                   \
    AESW_B2B_G(1, 6, 11, 12, w[s10], w[s11])                                                 \
    AESW_B2B_G(2, 7, 8, 13, w[s12], w[s13])                                                  \
    AESW_B2B_G(3, 4, 9, 14, w[s14], w[s15])

// h = F(h, m, t, last): one block of 16 little-endian words, t the bytes of the message up to and with this block
AESW_MONT_HD constexpr void blake2b_compress(uint64_t h[8], const uint64_t *m, uint64_t t, bool last) {
    const uint64_t w[16] = {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12], m[13], m[14], m[15]};
    uint64_t v[16] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], BLAKE2B_IV[0], BLAKE2B_IV[1], BLAKE2B_IV[2], BLAKE2B_IV[3],
                      BLAKE2B_IV[4] ^ t, BLAKE2B_IV[5], last ? ~BLAKE2B_IV[6] : BLAKE2B_IV[6], BLAKE2B_IV[7]};  // a message is below 2^64 bytes: the high counter word is 0
    AESW_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    AESW_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    AESW_B2B_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
    AESW_B2B_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
    AESW_B2B_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
    AESW_B2B_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
    AESW_B2B_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
    AESW_B2B_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
    AESW_B2B_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
    AESW_B2B_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
    AESW_B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    AESW_B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    AESW_MONT_UNROLL
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
#undef AESW_B2B_ROUND
#undef AESW_B2B_G

// ---- the state ----------------------------------------------------------------------------------------------------------------------
AESW_MONT_HD constexpr TranscriptState transcript_init() {
    TranscriptState s{};
    AESW_MONT_UNROLL
    for (int i = 0; i < 8; ++i) s.h[i] = BLAKE2B_IV[i];
    s.h[0] ^= BLAKE2B_PARAM0;
    s.h[6] ^= TRANSCRIPT_PERSON0;
    s.h[7] ^= TRANSCRIPT_PERSON1;
    s.first_identity = ~0ull;
    return s;
}

// the bytes of word i of a block that lie below `fill`, as a mask
AESW_MONT_HD constexpr uint64_t transcript_word_mask(uint64_t fill, uint32_t i) {
    const uint64_t first = 8ull * i;
    return fill >= first + 8 ? ~0ull : fill <= first ? 0ull : (1ull << (8 * (fill - first))) - 1;
}

// absorb with the lazy last block: a full block is compressed only when a further byte arrives
AESW_MONT_HD constexpr void transcript_absorb(TranscriptState &s, const uint8_t *bytes, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        if (s.fill == TRANSCRIPT_BLOCK) {
            s.count += TRANSCRIPT_BLOCK;
            blake2b_compress(s.h, s.block, s.count, false);
            s.fill = 0;
            AESW_MONT_UNROLL
            for (int w = 0; w < 16; ++w) s.block[w] = 0;  // the bytes from `fill` on are zero
        }
        const uint32_t at = (uint32_t)s.fill, shift = 8 * (at % 8);
        s.block[at / 8] = (s.block[at / 8] & ~(0xffull << shift) & transcript_word_mask(at, at / 8)) | ((uint64_t)bytes[i] << shift);
        s.fill = at + 1;
    }
}

// The same over a stream of whole words, as a workgroup holds it in LDS: `total` bytes (the bytes the state kept in front, 1 ... )
// lie from stream[0] on; every full block but the last is compressed; returns the bytes consumed, a multiple of 128 with
// 1 <= total - consumed <= 128.  The caller moves the remainder to the front and goes on.
AESW_MONT_HD constexpr uint32_t transcript_stream_blocks(uint64_t h[8], uint64_t &count, const uint64_t *stream, uint32_t total) {
    uint32_t at = 0;
    while (total - at > TRANSCRIPT_BLOCK) {
        count += TRANSCRIPT_BLOCK;
        blake2b_compress(h, stream + at / 8, count, false);
        at += TRANSCRIPT_BLOCK;
    }
    return at;
}

// the digest of what the state has absorbed, the state itself untouched: the last block, zero behind `fill`, with the final flag
AESW_MONT_HD constexpr void transcript_finalize_copy(const TranscriptState &s, uint64_t digest[8]) {
    uint64_t m[16] = {};
    AESW_MONT_UNROLL
    for (int i = 0; i < 16; ++i) m[i] = s.block[i] & transcript_word_mask(s.fill, i);
    AESW_MONT_UNROLL
    for (int i = 0; i < 8; ++i) digest[i] = s.h[i];
    blake2b_compress(digest, m, s.count + s.fill, true);
}

// ---- a 512-bit digest as a challenge ------------------------------------------------------------------------------------------------
// 2^512 mod r and 2^768 mod r: mont_mul by R^2 takes a plain value to its Montgomery form, by R^3 that of the value times 2^256
constexpr Fr FR_R2 = {{0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u}};
constexpr Fr FR_R3 = {{0xb4bf0040u, 0x5e94d8e1u, 0x1cfbb6b8u, 0x2a489cbeu, 0xa19fcfedu, 0x893cc664u, 0x7fcc657cu, 0x0cf8594bu}};
static_assert(mont_is_canonical(FR_R2) && mont_eq(mont_mul(FR_R2, FR_RAW_ONE), FR_ONE), "R^2 mod r: the Montgomery form of R");
static_assert(mont_is_canonical(FR_R3) && mont_eq(mont_mul(FR_R3, FR_RAW_ONE), FR_R2) && mont_eq(mont_mul(FR_R2, FR_R2), FR_R3), "R^3 mod r: the Montgomery form of R^2");

// One 256-bit half of a digest (four words) as its share of the cell: mont_mul(lo, R^2), or mont_mul(hi, R^3) for the high half.
// The half may be at or above r (the proof is at the top of this file).  The squeeze kernel gives the two halves to two lanes.
AESW_MONT_HD constexpr Fr fr_u512_half(const uint64_t *d, bool high) {
    const Fr half = {{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32), (uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)}};
    return mont_mul(half, mont_select(high, FR_R3, FR_R2));
}
// the digest as a little-endian integer mod r, as a cell
AESW_MONT_HD constexpr Fr fr_from_u512(const uint64_t d[8]) { return mont_add(fr_u512_half(d, false), fr_u512_half(d + 4, true)); }
constexpr Fr transcript_all_ones_cell() {
    const uint64_t d[8] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    return fr_from_u512(d);
}
static_assert(mont_is_canonical(transcript_all_ones_cell()) &&
                  mont_eq(transcript_all_ones_cell(), Fr{{0x54bf0046u, 0xf5e09a59u, 0xf7545a1fu, 0x1b800e70u, 0xaaa7e21cu, 0xdb1e68abu, 0xc6f62676u, 0x2f522ffcu}}),
              "(2^512 - 1) mod r as a cell: both halves at 2^256 - 1, above r");

// squeeze_challenge: 0x00 absorbed into the live state, a copy finalised to the digest; the digest reduced
AESW_MONT_HD constexpr void transcript_squeeze_digest(TranscriptState &s, uint64_t digest[8]) {
    const uint8_t tag[1] = {TRANSCRIPT_TAG_CHALLENGE};
    transcript_absorb(s, tag, 1);
    transcript_finalize_copy(s, digest);
}
AESW_MONT_HD constexpr Fr transcript_squeeze(TranscriptState &s) {
    uint64_t digest[8] = {};
    transcript_squeeze_digest(s, digest);
    return fr_from_u512(digest);
}
constexpr Fr transcript_first_challenge() {
    TranscriptState s = transcript_init();
    return transcript_squeeze(s);
}
static_assert(mont_eq(transcript_first_challenge(), Fr{{0x7da9a625u, 0x3c49925du, 0x0a0dec42u, 0x0b56f8acu, 0x3c823c30u, 0x1a8d03edu, 0xeabf601au, 0x0faad4aeu}}),
              "a squeeze straight after init: blake2b(person = Halo2-Transcript) of the one byte 0x00, mod r, as a cell");

// ---- the messages -------------------------------------------------------------------------------------------------------------------
// the plain value of a Montgomery form: one product with the raw 1 (msm_canonical_scalar's move); canonical for any a < 2^256
template <class F>
AESW_MONT_HD constexpr F transcript_plain(const F &v) {
    return mont_mul(v, MontField<F>::RAW_ONE);
}
// the 32 little-endian bytes of a plain value
template <class F>
AESW_MONT_HD constexpr void transcript_put(uint8_t *out, const F &plain) {
    AESW_MONT_UNROLL
    for (int i = 0; i < 4 * MONT_LIMBS; ++i) out[i] = (uint8_t)(plain.l[i / 4] >> (8 * (i % 4)));
}
AESW_MONT_HD constexpr bool transcript_is_identity(const Fq &x, const Fq &y) { return mont_is_zero(x) && mont_is_zero(y); }
// x and y in Montgomery form, as a point lies in memory
AESW_MONT_HD constexpr void point_message(const Fq &x, const Fq &y, uint8_t out[TRANSCRIPT_POINT_MESSAGE]) {
    out[0] = TRANSCRIPT_TAG_POINT;
    transcript_put(out + 1, transcript_plain(x));
    transcript_put(out + 33, transcript_plain(y));
}
AESW_MONT_HD constexpr void scalar_message(const Fr &cell, uint8_t out[TRANSCRIPT_SCALAR_MESSAGE]) {
    out[0] = TRANSCRIPT_TAG_SCALAR;
    transcript_put(out + 1, transcript_plain(cell));
}
// the sign of y into the top bit of the plain x (x < q < 2^254 leaves it free)
AESW_MONT_HD constexpr Fq transcript_compress_x(const Fq &plain_x, uint32_t y_low_limb) {
    Fq c = plain_x;
    c.l[MONT_LIMBS - 1] |= (y_low_limb & 1u) << 31;
    return c;
}
AESW_MONT_HD constexpr void point_compressed(const Fq &x, const Fq &y, uint8_t out[TRANSCRIPT_PROOF_ITEM]) {
    transcript_put(out, transcript_compress_x(transcript_plain(x), transcript_plain(y).l[0]));
}

}  // namespace aesw
