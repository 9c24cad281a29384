// aesw_fr.h -- bn256's scalar field Fr in Montgomery form, once, for host and device: the arithmetic behind the compression of
// the lookup arguments under theta (theta/aesw_theta.hip) and the lookup grand product (grand/aesw_grand.hip, 4.20).
// A cell is 32 bytes: eight little-endian 32-bit limbs of v * 2^256 mod r -- the encoding of every Fr cell the project writes
// (d_fr_lut of aesw_ctx.h holds the 256 byte values in this form), so a cell is loaded and stored as it lies.
// fr_mul is the Montgomery product a * b / 2^256 mod r, CIOS over 32-bit limbs: every step is a uint64_t accumulation of
// uint32_t products, which hipcc turns into 64-bit multiply-adds (v_mad_u64_u32) without a line of assembly.
// fr_unrolled<N>(f) is the unroll of every loop over an array of cells, for host and device as well.
// constexpr, no HIP call, no ROCm include and no other header of the project: tests/test_fr_header.py compiles this header
// alone with g++ and holds it against Python integers.
#pragma once
#include <stdint.h>

#include <utility>

#if defined(__HIPCC__)
#define AESW_FR_HD __host__ __device__ __forceinline__
#define AESW_FR_UNROLL _Pragma("unroll")  // limbs stay in registers: every index is a constant
#else
#define AESW_FR_HD inline
#define AESW_FR_UNROLL
#endif

namespace aesw {

constexpr int FR_LIMBS = 8;
struct Fr {
    uint32_t l[FR_LIMBS];
};

// r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
constexpr Fr FR_MODULUS = {{0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
constexpr Fr FR_ZERO = {{0, 0, 0, 0, 0, 0, 0, 0}};
// -r^-1 mod 2^32, by Newton's iteration on the lowest limb (five steps double 1 correct bit to 32)
constexpr uint32_t fr_neg_inverse(uint32_t r0) {
    uint32_t x = 1;
    for (int i = 0; i < 5; ++i) x *= 2u - r0 * x;
    return 0u - x;
}
constexpr uint32_t FR_INV = fr_neg_inverse(FR_MODULUS.l[0]);
static_assert(FR_INV == 0xefffffffu && (uint32_t)(FR_MODULUS.l[0] * FR_INV) == 0xffffffffu, "r * FR_INV == -1 mod 2^32");
static_assert(FR_MODULUS.l[FR_LIMBS - 1] < (1u << 30), "2 r < 2^255: a sum of two canonical values and the CIOS carry limb fit");

// a < r
AESW_FR_HD constexpr bool fr_is_canonical(const Fr &a) {
    bool below = false;  // decided by the highest limb that differs
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) below = a.l[i] < FR_MODULUS.l[i] || (a.l[i] == FR_MODULUS.l[i] && below);
    return below;
}

// t - r if t >= r, else t; t < 2 r, `top`: what of t lies above the eight limbs (0 or 1)
AESW_FR_HD constexpr Fr fr_reduce_once(const Fr &t, uint32_t top) {
    Fr d = FR_ZERO;
    uint64_t borrow = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) {
        const uint64_t v = (uint64_t)t.l[i] - FR_MODULUS.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const bool keep = borrow > top;  // t < r
    Fr out = FR_ZERO;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) out.l[i] = keep ? t.l[i] : d.l[i];
    return out;
}

// a + b mod r, both canonical
AESW_FR_HD constexpr Fr fr_add(const Fr &a, const Fr &b) {
    Fr t = FR_ZERO;
    uint64_t carry = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] + b.l[i] + carry;
        t.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return fr_reduce_once(t, (uint32_t)carry);
}

// a - b mod r, both canonical: the difference, and r added back where it borrowed (the transforms of aesw_ntt.h)
AESW_FR_HD constexpr Fr fr_sub(const Fr &a, const Fr &b) {
    Fr d = FR_ZERO;
    uint64_t borrow = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) {
        const uint64_t v = (uint64_t)a.l[i] - b.l[i] - borrow;
        d.l[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)borrow;  // all ones where a < b
    Fr out = FR_ZERO;
    uint64_t carry = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) {
        const uint64_t v = (uint64_t)d.l[i] + (FR_MODULUS.l[i] & mask) + carry;
        out.l[i] = (uint32_t)v;
        carry = v >> 32;
    }
    return out;
}

// a * b / 2^256 mod r, both canonical: the product of two Montgomery forms is the Montgomery form of the product
AESW_FR_HD constexpr Fr fr_mul(const Fr &a, const Fr &b) {
    uint32_t t[FR_LIMBS + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) {
        uint64_t c = 0;
        AESW_FR_UNROLL
        for (int j = 0; j < FR_LIMBS; ++j) {
            const uint64_t v = (uint64_t)a.l[j] * b.l[i] + t[j] + c;  // (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64
            t[j] = (uint32_t)v;
            c = v >> 32;
        }
        uint64_t v = (uint64_t)t[FR_LIMBS] + c;
        t[FR_LIMBS] = (uint32_t)v;
        t[FR_LIMBS + 1] = (uint32_t)(v >> 32);
        const uint32_t m = t[0] * FR_INV;
        c = ((uint64_t)m * FR_MODULUS.l[0] + t[0]) >> 32;  // the low word is 0 by the choice of m
        AESW_FR_UNROLL
        for (int j = 1; j < FR_LIMBS; ++j) {
            v = (uint64_t)m * FR_MODULUS.l[j] + t[j] + c;
            t[j - 1] = (uint32_t)v;
            c = v >> 32;
        }
        v = (uint64_t)t[FR_LIMBS] + c;
        t[FR_LIMBS - 1] = (uint32_t)v;
        t[FR_LIMBS] = t[FR_LIMBS + 1] + (uint32_t)(v >> 32);
    }
    Fr out = FR_ZERO;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) out.l[i] = t[i];
    return fr_reduce_once(out, t[FR_LIMBS]);
}

// 2^256 mod r: the Montgomery form of 1
constexpr Fr FR_ONE = {{0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};
static_assert(fr_is_canonical(FR_ONE) && fr_mul(FR_ONE, FR_ONE).l[0] == FR_ONE.l[0] && fr_mul(FR_ONE, FR_ONE).l[7] == FR_ONE.l[7],
              "the Montgomery form of 1 is the identity of fr_mul");

AESW_FR_HD constexpr bool fr_is_zero(const Fr &a) {
    uint32_t any = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) any |= a.l[i];
    return any == 0;
}
// limb for limb: canonical cells are equal as field elements exactly when they are
AESW_FR_HD constexpr bool fr_eq(const Fr &a, const Fr &b) {
    uint32_t any = 0;
    AESW_FR_UNROLL
    for (int i = 0; i < FR_LIMBS; ++i) any |= a.l[i] ^ b.l[i];
    return any == 0;
}

// a^(r - 2): the inverse of a canonical a in Montgomery form (Fermat), and 0 for 0 -- the convention of ff's batch_invert.
// A fixed square-and-multiply over the constant exponent, highest bit first, by loops that stay loops (two products of code; 256
// squarings and one product per set bit of time); the limb of the exponent is chosen among constants, not read from an array.
// One call per batch of a Montgomery inversion (aesw_grand.h), never one per cell.
AESW_FR_HD constexpr uint32_t fr_inv_exponent_limb(int i) {  // limb i of r - 2: the lowest limb of r is above 2, nothing borrows
    return i == 0 ? FR_MODULUS.l[0] - 2u : i == 1 ? FR_MODULUS.l[1] : i == 2 ? FR_MODULUS.l[2] : i == 3 ? FR_MODULUS.l[3] : i == 4 ? FR_MODULUS.l[4]
         : i == 5 ? FR_MODULUS.l[5] : i == 6 ? FR_MODULUS.l[6] : FR_MODULUS.l[7];
}
AESW_FR_HD constexpr Fr fr_inv(const Fr &a) {
    Fr acc = FR_ONE;
    for (int i = FR_LIMBS - 1; i >= 0; --i) {
        const uint32_t e = fr_inv_exponent_limb(i);
        for (int b = 31; b >= 0; --b) {
            acc = fr_mul(acc, acc);
            if (e >> b & 1u) acc = fr_mul(acc, a);
        }
    }
    return acc;
}
// one evaluation at compile time (380 products); fr_inv(0) == 0 and the rest are tests/test_fr_inverse.py's
static_assert(FR_MODULUS.l[0] >= 2u && fr_eq(fr_mul(fr_inv(fr_add(FR_ONE, FR_ONE)), fr_add(FR_ONE, FR_ONE)), FR_ONE), "fr_inv(2) * 2 is 1");

// f(i) for i = 0 ... N - 1 with i a constant of the type system (decltype(i)::value): a pack expansion, not a loop.  A loop whose
// body holds field products is too large for the compiler to unroll on request, and a cell array indexed by a loop that
// stays a loop leaves the registers for scratch memory.
template <class F, int... I>
AESW_FR_HD void fr_each(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
AESW_FR_HD void fr_unrolled(F &&f) {
    fr_each(f, std::make_integer_sequence<int, N>{});
}

// The 256 byte values as cells, cell v = v * 2^256 mod r: what d_fr_lut (aesw_ctx.h) holds on the device and what the columns
// checker inverts (aesw_cols_fr_table).  Little-endian limbs: on the hosts the project builds for, the table's bytes as they lie.
struct FrByteTable {
    Fr cell[256];
};
constexpr FrByteTable fr_byte_table() {
    FrByteTable t{};
    Fr acc = FR_ZERO;
    for (int v = 0; v < 256; ++v) {
        t.cell[v] = acc;
        acc = fr_add(acc, FR_ONE);
    }
    return t;
}
static_assert(fr_byte_table().cell[0].l[0] == 0 && fr_byte_table().cell[0].l[7] == 0 && fr_byte_table().cell[1].l[0] == FR_ONE.l[0] &&
                  fr_byte_table().cell[1].l[7] == FR_ONE.l[7],
              "cells 0 and 1 are the Montgomery forms of 0 and 1");
static_assert(fr_byte_table().cell[255].l[0] == 0x3ffffabcu && fr_byte_table().cell[255].l[3] == 0x4eace25fu && fr_byte_table().cell[255].l[7] == 0x2fd2eb16u,
              "cell 255 is 255 * 2^256 mod r");

}  // namespace aesw
