// aesw_blind.h -- the rules of libaesw_blind.so, once: the cells a prover blinds the last rows of a column with, and
// the commitment of a column of bytes whose tail is such cells -- for the kernels of blind/aesw_blind.hip and for the CPU driver of
// tests/blind_driver.cpp.  Blake2b and the wide reduction are aesw_transcript.h's, the group and its law aesw_msm.h's, the fields
// aesw_fr.h's and aesw_fq.h's; nothing of them is restated.  No HIP call and no ROCm include: tests/test_blind_model.py compiles this
// header alone with g++.
//
// THE CELL is a pure function of (seed, domain, column, row):
//   digest = BLAKE2b-512(key = seed[32], person = "aesw-blind-cells", message = le64(domain) || le64(column) || le64(row))
//   cell   = fr_from_u512(digest): the 64 bytes as a little-endian integer mod r, in Montgomery form, canonical
// exactly as Python's hashlib.blake2b(message, key=seed, person=b"aesw-blind-cells", digest_size=64) computes the digest
// (tests/blind_model.py): keyed Blake2b compresses the key, padded with zeros to one block of 128 bytes, first (t = 128), then the
// 24-byte message, padded to a block, with the final flag (t = 152).  The parameter block's word 0 carries the digest length 64, the
// key length 32, fanout 1 and depth 1; words 6 and 7 the person.  The wide reduction is what halo2curves' Fr::random does with 64
// bytes: its bias is below 2^-256.  `domain` is the caller's tag for a group of columns, so groups under one seed share no cell.
// Determinism is the contract: a proof is reproducible from its seed, and the randomness is the seed's, which the host draws.
// Which rows of which column a prover blinds is the caller's first_row; parity with halo2's own RNG stream is not a goal.
//
// THE TAIL COMMITMENT.  C += sum_(i >= first_row) tail[i - first_row] * P_i for at most BLIND_MAX_TAIL rows.  A term is blind_term: a
// fixed 254-step double-and-add over the canonical scalar, highest bit first, where the bit decides by msm_select and never by a
// branch -- the scalars are secret, and the lanes of a wave stay in lockstep.  The scalar is shifted as a whole each step, so every
// limb index is a constant.  The terms and the old commitment are added by the complete law, in any order: the law is exact and the
// group commutative, so the affine result is the same bytes.
#pragma once
#include <stdint.h>

#include "aesw_msm.h"
#include "aesw_transcript.h"

namespace aesw {

constexpr uint32_t BLIND_MIN_K = 10, BLIND_MAX_K = 28, BLIND_MAX_COLS = 65535;
constexpr uint32_t BLIND_SEED_BYTES = 32, BLIND_MESSAGE_BYTES = 24;
constexpr uint32_t BLIND_MAX_TAIL = 64;  // the most tail rows the commit call takes: a lane of one wave each
constexpr uint32_t BLIND_SCALAR_BITS = 254;  // r < 2^254
static_assert(BLIND_MIN_K == MSM_MIN_K && BLIND_MAX_K == MSM_MAX_K && BLIND_MAX_COLS == MSM_MAX_COLS, "the bounds of a commitment are libaesw_msm.so's");
static_assert(BLIND_MAX_TAIL == MSM_LANES, "one lane per tail row");
static_assert(FR_MODULUS.l[FR_LIMBS - 1] >> 30 == 0 && FR_MODULUS.l[FR_LIMBS - 1] >> 29 == 1, "r has 254 bits");

constexpr bool blind_k_ok(uint32_t k) { return k >= BLIND_MIN_K && k <= BLIND_MAX_K; }
constexpr bool blind_cols_ok(uint32_t n_cols) { return n_cols >= 1 && n_cols <= BLIND_MAX_COLS; }
constexpr bool blind_first_row_ok(uint32_t k, uint64_t first_row) { return first_row < ((uint64_t)1 << k); }
// the rows from first_row on, 0 outside the bounds
constexpr uint64_t blind_tail_rows(uint32_t k, uint64_t first_row) { return blind_k_ok(k) && blind_first_row_ok(k, first_row) ? ((uint64_t)1 << k) - first_row : 0u; }
constexpr bool blind_commit_tail_ok(uint32_t k, uint64_t first_row) { return blind_tail_rows(k, first_row) >= 1 && blind_tail_rows(k, first_row) <= BLIND_MAX_TAIL; }
static_assert(blind_tail_rows(10, 1018) == 6 && blind_tail_rows(10, 0) == 1024 && blind_tail_rows(10, 1024) == 0 && blind_tail_rows(9, 0) == 0 && blind_tail_rows(29, 0) == 0 &&
                  blind_commit_tail_ok(10, 960) && !blind_commit_tail_ok(10, 959),
              "the tail: 2^k - first_row rows, at most 64 of them for the commitment");

// ---- the hash ----------------------------------------------------------------------------------------------------------------------
// the parameter block: digest length 64, key length 32, fanout 1, depth 1 in word 0; the 16 bytes of the person in words 6 and 7
constexpr uint64_t BLIND_PARAM0 = 0x01012040ull, BLIND_PERSON0 = 0x696c622d77736561ull /* "aesw-bli" */, BLIND_PERSON1 = 0x736c6c65632d646eull /* "nd-cells" */;

// the chain value after the key block: the same for every cell of a seed
struct BlindKey {
    uint64_t h[8];
};
// seed: the 32 bytes as four little-endian words
AESW_MONT_HD constexpr BlindKey blind_key(const uint64_t seed[4]) {
    BlindKey key{};
    AESW_MONT_UNROLL
    for (int i = 0; i < 8; ++i) key.h[i] = BLAKE2B_IV[i];
    key.h[0] ^= BLIND_PARAM0;
    key.h[6] ^= BLIND_PERSON0;
    key.h[7] ^= BLIND_PERSON1;
    const uint64_t block[16] = {seed[0], seed[1], seed[2], seed[3], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    blake2b_compress(key.h, block, TRANSCRIPT_BLOCK, false);
    return key;
}
AESW_MONT_HD constexpr void blind_digest(const BlindKey &key, uint64_t domain, uint64_t column, uint64_t row, uint64_t digest[8]) {
    AESW_MONT_UNROLL
    for (int i = 0; i < 8; ++i) digest[i] = key.h[i];
    const uint64_t block[16] = {domain, column, row, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    blake2b_compress(digest, block, TRANSCRIPT_BLOCK + BLIND_MESSAGE_BYTES, true);
}
AESW_MONT_HD constexpr Fr blind_cell(const BlindKey &key, uint64_t domain, uint64_t column, uint64_t row) {
    uint64_t digest[8] = {};
    blind_digest(key, domain, column, row, digest);
    return fr_from_u512(digest);
}
constexpr Fr blind_fixed_cell() {
    const uint64_t seed[4] = {0x0706050403020100ull, 0x0f0e0d0c0b0a0908ull, 0x1716151413121110ull, 0x1f1e1d1c1b1a1918ull};
    return blind_cell(blind_key(seed), 1, 2, 3);
}
static_assert(mont_is_canonical(blind_fixed_cell()) &&
                  mont_eq(blind_fixed_cell(), Fr{{0x040d7cb5u, 0x10227b6au, 0xa02b4317u, 0xb9f0c6e5u, 0x0841bf58u, 0xf54457deu, 0x87289c43u, 0x1837c340u}}),
              "hashlib.blake2b(le64(1) + le64(2) + le64(3), key=bytes(range(32)), person=b'aesw-blind-cells', digest_size=64), mod r, as a cell");

// ---- a term of the tail commitment -------------------------------------------------------------------------------------------------
// cell * p: 254 doublings and 254 mixed additions whatever the scalar; the bit selects
AESW_MONT_HD constexpr G1 blind_term(const Fr &cell, const G1Affine &p) {
    Fr s = msm_canonical_scalar(cell);
    // bit 253 to the top of the top limb
    AESW_MONT_UNROLL
    for (int i = FR_LIMBS - 1; i > 0; --i) s.l[i] = (s.l[i] << 2) | (s.l[i - 1] >> 30);
    s.l[0] <<= 2;
    G1 acc = msm_identity();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t step = 0; step < BLIND_SCALAR_BITS; ++step) {
        const bool bit = (s.l[FR_LIMBS - 1] >> 31) != 0;
        AESW_MONT_UNROLL
        for (int i = FR_LIMBS - 1; i > 0; --i) s.l[i] = (s.l[i] << 1) | (s.l[i - 1] >> 31);
        s.l[0] <<= 1;
        acc = msm_double(acc);
        acc = msm_select(bit, msm_add_mixed(acc, p), acc);
    }
    return acc;
}

}  // namespace aesw
