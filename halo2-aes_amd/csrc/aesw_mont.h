// aesw_mont.h -- Montgomery arithmetic over eight 32-bit limbs, once, for host and device and for every field of the project:
// bn256's scalar field Fr (aesw_fr.h) and its base field Fq (aesw_fq.h).  A value is 32 bytes: eight little-endian 32-bit limbs of
// v * 2^256 mod m.  mont_mul is the Montgomery product a * b / 2^256 mod m, CIOS over 32-bit limbs: every step is a uint64_t
// accumulation of uint32_t products, which hipcc turns into 64-bit multiply-adds (v_mad_u64_u32) from plain C++.
// A field is a plain struct F of eight uint32_t `l` and a specialisation MontField<F> with its constants: MODULUS, INV = -m^-1 mod
// 2^32, ZERO, RAW_ONE (the plain 1) and ONE (2^256 mod m, the Montgomery form of 1).  The field is deduced from the arguments.
// Each field's header names the instantiations by references (fr_mul, fq_mul ...), not by forwarding functions: a function layer
// over these templates changes what hipcc emits for the kernels (profiles/mont_core/README.md).
// constexpr, no HIP call, no ROCm include and no header of the project: tests/test_field_headers.py compiles it behind each
// field's header with g++ and holds it against Python integers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AESW_MONT_HD __host__ __device__ __forceinline__
#define AESW_MONT_UNROLL _Pragma("unroll")  // limbs stay in registers: every index is a constant
#else
#define AESW_MONT_HD inline
#define AESW_MONT_UNROLL
#endif

namespace aesw {

constexpr int MONT_LIMBS = 8;
template <class F>
struct MontField;  // each field's header specialises it

// -m^-1 mod 2^32, by Newton's iteration on the lowest limb (five steps double 1 correct bit to 32)
constexpr uint32_t mont_neg_inverse(uint32_t m0) {
    uint32_t x = 1;
    for (int i = 0; i < 5; ++i) x *= 2u - m0 * x;
    return 0u - x;
}

// a < m
template <class F>
AESW_MONT_HD constexpr bool mont_is_canonical(const F &a) {
    using M = MontField<F>;
    bool below = false;  // decided by the highest limb that differs
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) below = a.l[i] < M::MODULUS.l[i] || (a.l[i] == M::MODULUS.l[i] && below);
    return below;
}

// t - m if t >= m, else t; t < 2 m, `top`: what of t lies above the eight limbs (0 or 1)
template <class F>
AESW_MONT_HD constexpr F mont_reduce_once(const F &t, uint32_t top) {
    using M = MontField<F>;
    static_assert(sizeof(F) == 4 * MONT_LIMBS, "a field element is eight 32-bit limbs and nothing else");
    static_assert(M::MODULUS.l[MONT_LIMBS - 1] < (1u << 30), "2 m < 2^255: a sum of two canonical values and the CIOS carry limb fit");
    F d = M::ZERO;
    uint64_t borrow = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) {
        const uint64_t v = (uint64_t)t.l[i] - M::MODULUS.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const bool keep = borrow > top;  // t < m
    F out = M::ZERO;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) out.l[i] = keep ? t.l[i] : d.l[i];
    return out;
}

// a + b mod m, both canonical
template <class F>
AESW_MONT_HD constexpr F mont_add(const F &a, const F &b) {
    using M = MontField<F>;
    F t = M::ZERO;
    uint64_t carry = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] + b.l[i] + carry;
        t.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return mont_reduce_once(t, (uint32_t)carry);
}

// a - b mod m, both canonical: the difference, and m added back where it borrowed (the transforms of aesw_ntt.h)
template <class F>
AESW_MONT_HD constexpr F mont_sub(const F &a, const F &b) {
    using M = MontField<F>;
    F d = M::ZERO;
    uint64_t borrow = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] - b.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)borrow;  // all ones where a < b
    F out = M::ZERO;
    uint64_t carry = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) {
        const uint64_t v = (uint64_t)d.l[i] + (M::MODULUS.l[i] & mask) + carry;
        out.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return out;
}

// a * b / 2^256 mod m, both canonical: the product of two Montgomery forms is the Montgomery form of the product
template <class F>
AESW_MONT_HD constexpr F mont_mul(const F &a, const F &b) {
    using M = MontField<F>;
    static_assert((uint32_t)(M::MODULUS.l[0] * M::INV) == 0xffffffffu, "m * INV == -1 mod 2^32");
    uint32_t t[MONT_LIMBS + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) {
        uint64_t c = 0;
        AESW_MONT_UNROLL
        for (int j = 0; j < MONT_LIMBS; ++j) {
            const uint64_t v = (uint64_t)a.l[j] * b.l[i] + t[j] + c;  // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            t[j] = (uint32_t)v;
            c = v >> 32;
        }
        uint64_t v = (uint64_t)t[MONT_LIMBS] + c;
        t[MONT_LIMBS] = (uint32_t)v;
        t[MONT_LIMBS + 1] = (uint32_t)(v >> 32);
        const uint32_t m = t[0] * M::INV;
        c = ((uint64_t)m * M::MODULUS.l[0] + t[0]) >> 32;  // the low word is 0 by the choice of m
        AESW_MONT_UNROLL
        for (int j = 1; j < MONT_LIMBS; ++j) {
            v = (uint64_t)m * M::MODULUS.l[j] + t[j] + c;
            t[j - 1] = (uint32_t)v;
            c = v >> 32;
        }
        v = (uint64_t)t[MONT_LIMBS] + c;
        t[MONT_LIMBS - 1] = (uint32_t)v;
        t[MONT_LIMBS] = t[MONT_LIMBS + 1] + (uint32_t)(v >> 32);
    }
    F out = M::ZERO;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) out.l[i] = t[i];
    return mont_reduce_once(out, t[MONT_LIMBS]);
}

template <class F>
AESW_MONT_HD constexpr bool mont_is_zero(const F &a) {
    uint32_t any = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) any |= a.l[i];
    return any == 0;
}
// limb for limb: canonical values are equal as field elements exactly when they are
template <class F>
AESW_MONT_HD constexpr bool mont_eq(const F &a, const F &b) {
    uint32_t any = 0;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) any |= a.l[i] ^ b.l[i];
    return any == 0;
}
// a where take, else b: every limb chosen, no branch
template <class F>
AESW_MONT_HD constexpr F mont_select(bool take, const F &a, const F &b) {
    using M = MontField<F>;
    F out = M::ZERO;
    AESW_MONT_UNROLL
    for (int i = 0; i < MONT_LIMBS; ++i) out.l[i] = take ? a.l[i] : b.l[i];
    return out;
}

// limb i of m - 2, the exponent of the inverse a^(m - 2) (Fermat): chosen among constants, not read from an array.  The lowest limb
// of m is above 2, so nothing borrows.  The square-and-multiply itself is each field's own (fr_inv, fq_inv).
template <class F>
AESW_MONT_HD constexpr uint32_t mont_inv_exponent_limb(int i) {
    using M = MontField<F>;
    static_assert(M::MODULUS.l[0] >= 2u, "m - 2 does not borrow");
    return i == 0 ? M::MODULUS.l[0] - 2u : i == 1 ? M::MODULUS.l[1] : i == 2 ? M::MODULUS.l[2] : i == 3 ? M::MODULUS.l[3]
         : i == 4 ? M::MODULUS.l[4] : i == 5 ? M::MODULUS.l[5] : i == 6 ? M::MODULUS.l[6] : M::MODULUS.l[7];
}

}  // namespace aesw
