// aesw_fq.h -- bn256's base field Fq in Montgomery form, once, for host and device: the coordinates of the points of G1 behind the
// commitments of msm/aesw_msm.hip.  Written as aesw_fr.h is, limb for limb: a coordinate is 32 bytes, eight
// little-endian 32-bit limbs of v * 2^256 mod q; fq_mul is the Montgomery product a * b / 2^256 mod q, CIOS over 32-bit limbs,
// every step a uint64_t accumulation of uint32_t products (v_mad_u64_u32 on the device).  The two fields share nothing here: one
// Montgomery template for both is a refactor of its own (aesw_fr.h is what the tracked ISA tables of seven libraries hang on).
// constexpr, no HIP call, no ROCm include and no other header of the project: tests/test_fq_header.py compiles this header
// alone with g++ and holds it against Python integers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AESW_FQ_HD __host__ __device__ __forceinline__
#define AESW_FQ_UNROLL _Pragma("unroll")  // limbs stay in registers: every index is a constant
#else
#define AESW_FQ_HD inline
#define AESW_FQ_UNROLL
#endif

namespace aesw {

constexpr int FQ_LIMBS = 8;
struct Fq {
    uint32_t l[FQ_LIMBS];
};

// q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
constexpr Fq FQ_MODULUS = {{0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
constexpr Fq FQ_ZERO = {{0, 0, 0, 0, 0, 0, 0, 0}};
// -q^-1 mod 2^32, by Newton's iteration on the lowest limb (five steps double 1 correct bit to 32)
constexpr uint32_t fq_neg_inverse(uint32_t q0) {
    uint32_t x = 1;
    for (int i = 0; i < 5; ++i) x *= 2u - q0 * x;
    return 0u - x;
}
constexpr uint32_t FQ_INV = fq_neg_inverse(FQ_MODULUS.l[0]);
static_assert(FQ_INV == 0xe4866389u && (uint32_t)(FQ_MODULUS.l[0] * FQ_INV) == 0xffffffffu, "q * FQ_INV == -1 mod 2^32");
static_assert(FQ_MODULUS.l[FQ_LIMBS - 1] < (1u << 30), "2 q < 2^255: a sum of two canonical values and the CIOS carry limb fit");

// a < q
AESW_FQ_HD constexpr bool fq_is_canonical(const Fq &a) {
    bool below = false;  // decided by the highest limb that differs
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) below = a.l[i] < FQ_MODULUS.l[i] || (a.l[i] == FQ_MODULUS.l[i] && below);
    return below;
}

// t - q if t >= q, else t; t < 2 q, `top`: what of t lies above the eight limbs (0 or 1)
AESW_FQ_HD constexpr Fq fq_reduce_once(const Fq &t, uint32_t top) {
    Fq d = FQ_ZERO;
    uint64_t borrow = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) {
        const uint64_t v = (uint64_t)t.l[i] - FQ_MODULUS.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const bool keep = borrow > top;  // t < q
    Fq out = FQ_ZERO;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) out.l[i] = keep ? t.l[i] : d.l[i];
    return out;
}

// a + b mod q, both canonical
AESW_FQ_HD constexpr Fq fq_add(const Fq &a, const Fq &b) {
    Fq t = FQ_ZERO;
    uint64_t carry = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] + b.l[i] + carry;
        t.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return fq_reduce_once(t, (uint32_t)carry);
}

// a - b mod q, both canonical: the difference, and q added back where it borrowed
AESW_FQ_HD constexpr Fq fq_sub(const Fq &a, const Fq &b) {
    Fq d = FQ_ZERO;
    uint64_t borrow = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] - b.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)borrow;  // all ones where a < b
    Fq out = FQ_ZERO;
    uint64_t carry = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) {
        const uint64_t v = (uint64_t)d.l[i] + (FQ_MODULUS.l[i] & mask) + carry;
        out.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return out;
}

// a * b / 2^256 mod q, both canonical: the product of two Montgomery forms is the Montgomery form of the product
AESW_FQ_HD constexpr Fq fq_mul(const Fq &a, const Fq &b) {
    uint32_t t[FQ_LIMBS + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) {
        uint64_t c = 0;
        AESW_FQ_UNROLL
        for (int j = 0; j < FQ_LIMBS; ++j) {
            const uint64_t v = (uint64_t)a.l[j] * b.l[i] + t[j] + c;  // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            t[j] = (uint32_t)v;
            c = v >> 32;
        }
        uint64_t v = (uint64_t)t[FQ_LIMBS] + c;
        t[FQ_LIMBS] = (uint32_t)v;
        t[FQ_LIMBS + 1] = (uint32_t)(v >> 32);
        const uint32_t m = t[0] * FQ_INV;
        c = ((uint64_t)m * FQ_MODULUS.l[0] + t[0]) >> 32;  // the low word is 0 by the choice of m
        AESW_FQ_UNROLL
        for (int j = 1; j < FQ_LIMBS; ++j) {
            v = (uint64_t)m * FQ_MODULUS.l[j] + t[j] + c;
            t[j - 1] = (uint32_t)v;
            c = v >> 32;
        }
        v = (uint64_t)t[FQ_LIMBS] + c;
        t[FQ_LIMBS - 1] = (uint32_t)v;
        t[FQ_LIMBS] = t[FQ_LIMBS + 1] + (uint32_t)(v >> 32);
    }
    Fq out = FQ_ZERO;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) out.l[i] = t[i];
    return fq_reduce_once(out, t[FQ_LIMBS]);
}

AESW_FQ_HD constexpr bool fq_is_zero(const Fq &a) {
    uint32_t any = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) any |= a.l[i];
    return any == 0;
}
// limb for limb: canonical values are equal as field elements exactly when they are
AESW_FQ_HD constexpr bool fq_eq(const Fq &a, const Fq &b) {
    uint32_t any = 0;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) any |= a.l[i] ^ b.l[i];
    return any == 0;
}
// a where take, else b: every limb chosen, no branch
AESW_FQ_HD constexpr Fq fq_select(bool take, const Fq &a, const Fq &b) {
    Fq out = FQ_ZERO;
    AESW_FQ_UNROLL
    for (int i = 0; i < FQ_LIMBS; ++i) out.l[i] = take ? a.l[i] : b.l[i];
    return out;
}

constexpr Fq FQ_RAW_ONE = {{1, 0, 0, 0, 0, 0, 0, 0}};  // fq_mul by it takes a Montgomery form to the plain value
// 2^256 mod q: the Montgomery form of 1
constexpr Fq FQ_ONE = {{0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};
// 2^512 mod q: fq_mul by it takes a plain value to its Montgomery form
constexpr Fq FQ_R2 = {{0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}};
// 3 * 2^256 mod q: the curve's b in Montgomery form
constexpr Fq FQ_THREE = {{0x50ad28d7u, 0x7a17caa9u, 0xe15521b9u, 0x1f6ac17au, 0x696bd284u, 0x334bea4eu, 0xce179d8eu, 0x2a1f6744u}};
static_assert(fq_is_canonical(FQ_ONE) && fq_eq(fq_mul(FQ_ONE, FQ_ONE), FQ_ONE) && fq_eq(fq_mul(FQ_ONE, FQ_RAW_ONE), FQ_RAW_ONE),
              "R mod q: the Montgomery form of 1 is the identity of fq_mul, and its plain value is 1");
static_assert(fq_is_canonical(FQ_R2) && fq_eq(fq_mul(FQ_R2, FQ_RAW_ONE), FQ_ONE), "R^2 mod q: the Montgomery form of R");
static_assert(fq_is_canonical(FQ_THREE) && fq_eq(fq_add(fq_add(FQ_ONE, FQ_ONE), FQ_ONE), FQ_THREE), "3 R mod q");

// a^(q - 2): the inverse of a canonical a in Montgomery form (Fermat), and 0 for 0.  A fixed square-and-multiply over the
// constant exponent, highest bit first, by loops that stay loops; the limb of the exponent is chosen among constants, not read
// from an array.  One call per commitment (the projective result made affine), never one per addition.
AESW_FQ_HD constexpr uint32_t fq_inv_exponent_limb(int i) {  // limb i of q - 2: the lowest limb of q is above 2, nothing borrows
    return i == 0 ? FQ_MODULUS.l[0] - 2u : i == 1 ? FQ_MODULUS.l[1] : i == 2 ? FQ_MODULUS.l[2] : i == 3 ? FQ_MODULUS.l[3] : i == 4 ? FQ_MODULUS.l[4]
         : i == 5 ? FQ_MODULUS.l[5] : i == 6 ? FQ_MODULUS.l[6] : FQ_MODULUS.l[7];
}
AESW_FQ_HD constexpr Fq fq_inv(const Fq &a) {
    Fq acc = FQ_ONE;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = FQ_LIMBS - 1; i >= 0; --i) {
        const uint32_t e = fq_inv_exponent_limb(i);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int b = 31; b >= 0; --b) {
            acc = fq_mul(acc, acc);
            const Fq with = fq_mul(acc, a);
            acc = fq_select(e >> b & 1u, with, acc);
        }
    }
    return acc;
}
static_assert(FQ_MODULUS.l[0] >= 2u && fq_eq(fq_mul(fq_inv(FQ_THREE), FQ_THREE), FQ_ONE) && fq_is_zero(fq_inv(FQ_ZERO)), "fq_inv(3) * 3 is 1; fq_inv(0) is 0");

}  // namespace aesw
