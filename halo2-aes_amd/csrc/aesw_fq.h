// aesw_fq.h -- bn256's base field Fq in Montgomery form, for host and device: the coordinates of the points of G1 behind the
// commitments of msm/aesw_msm.hip.  A coordinate is 32 bytes, eight little-endian 32-bit limbs of v * 2^256 mod q.
// The arithmetic is aesw_mont.h's, which Fr (aesw_fr.h) shares: fq_mul, fq_add, fq_sub, fq_select ... are its instantiations
// for Fq under the names every caller uses.  Here is what is Fq's own: the struct, the constants and the inverse.
// constexpr, no HIP call, no ROCm include and of the project aesw_mont.h alone: tests/test_field_headers.py compiles this header
// with g++ and holds it against Python integers.
#pragma once
#include <stdint.h>

#include "aesw_mont.h"

namespace aesw {

constexpr int FQ_LIMBS = MONT_LIMBS;
struct Fq {
    uint32_t l[FQ_LIMBS];
};

// q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
constexpr Fq FQ_MODULUS = {{0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
constexpr Fq FQ_ZERO = {{0, 0, 0, 0, 0, 0, 0, 0}};
constexpr uint32_t FQ_INV = mont_neg_inverse(FQ_MODULUS.l[0]);
static_assert(FQ_INV == 0xe4866389u, "-q^-1 mod 2^32");
constexpr Fq FQ_RAW_ONE = {{1, 0, 0, 0, 0, 0, 0, 0}};  // mont_mul by it takes a Montgomery form to the plain value
// 2^256 mod q: the Montgomery form of 1
constexpr Fq FQ_ONE = {{0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};
template <>
struct MontField<Fq> {
    static constexpr Fq MODULUS = FQ_MODULUS, ZERO = FQ_ZERO, RAW_ONE = FQ_RAW_ONE, ONE = FQ_ONE;
    static constexpr uint32_t INV = FQ_INV;
};
// 2^512 mod q: mont_mul by it takes a plain value to its Montgomery form
constexpr Fq FQ_R2 = {{0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}};
// 3 * 2^256 mod q: the curve's b in Montgomery form
constexpr Fq FQ_THREE = {{0x50ad28d7u, 0x7a17caa9u, 0xe15521b9u, 0x1f6ac17au, 0x696bd284u, 0x334bea4eu, 0xce179d8eu, 0x2a1f6744u}};
static_assert(mont_is_canonical(FQ_ONE) && mont_eq(mont_mul(FQ_ONE, FQ_ONE), FQ_ONE) && mont_eq(mont_mul(FQ_ONE, FQ_RAW_ONE), FQ_RAW_ONE),
              "R mod q: the Montgomery form of 1 is the identity of mont_mul, and its plain value is 1");
static_assert(mont_is_canonical(FQ_R2) && mont_eq(mont_mul(FQ_R2, FQ_RAW_ONE), FQ_ONE), "R^2 mod q: the Montgomery form of R");
static_assert(mont_is_canonical(FQ_THREE) && mont_eq(mont_add(mont_add(FQ_ONE, FQ_ONE), FQ_ONE), FQ_THREE), "3 R mod q");

// The core under Fq's names: references to its instantiations, resolved where they are named.  Not functions: a forwarding
// function per name is an inline layer of its own, and changes what hipcc emits for the kernels (profiles/mont_core/README.md).
inline constexpr auto &fq_is_canonical = mont_is_canonical<Fq>;
inline constexpr auto &fq_add = mont_add<Fq>;
inline constexpr auto &fq_sub = mont_sub<Fq>;
inline constexpr auto &fq_mul = mont_mul<Fq>;
inline constexpr auto &fq_is_zero = mont_is_zero<Fq>;
inline constexpr auto &fq_eq = mont_eq<Fq>;
inline constexpr auto &fq_select = mont_select<Fq>;

// a^(q - 2): the inverse of a canonical a in Montgomery form (Fermat), and 0 for 0.  A fixed square-and-multiply over the
// constant exponent, highest bit first, by loops that stay loops; the limb of the exponent is chosen among constants, not read
// from an array.  One call per commitment (the projective result made affine), never one per addition.
// Fq's own body, not the core's: it selects without a branch under loops held to one iteration a turn, where fr_inv branches on the bit.
AESW_MONT_HD constexpr Fq fq_inv(const Fq &a) {
    Fq acc = FQ_ONE;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = FQ_LIMBS - 1; i >= 0; --i) {
        const uint32_t e = mont_inv_exponent_limb<Fq>(i);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int b = 31; b >= 0; --b) {
            acc = mont_mul(acc, acc);
            const Fq with = mont_mul(acc, a);
            acc = mont_select(e >> b & 1u, with, acc);
        }
    }
    return acc;
}
static_assert(mont_eq(mont_mul(fq_inv(FQ_THREE), FQ_THREE), FQ_ONE) && mont_is_zero(fq_inv(FQ_ZERO)), "fq_inv(3) * 3 is 1; fq_inv(0) is 0");

}  // namespace aesw
