// aesw_fr.h -- bn256's scalar field Fr in Montgomery form, for host and device: the arithmetic behind the compression of
// the lookup arguments under theta (theta/aesw_theta.hip) and the lookup grand product (grand/aesw_grand.hip, 4.20).
// A cell is 32 bytes: eight little-endian 32-bit limbs of v * 2^256 mod r -- the encoding of every Fr cell the project writes
// (d_fr_lut of aesw_ctx.h holds the 256 byte values in this form), so a cell is loaded and stored as it lies.
// The arithmetic is aesw_mont.h's, which Fq (aesw_fq.h) shares: fr_mul, fr_add, fr_sub, fr_eq ... are its instantiations for Fr
// under the names every caller uses.  Here is what is Fr's own: the struct, the constants, the inverse, the unroll and the byte table.
// fr_unrolled<N>(f) is the unroll of every loop over an array of cells, for host and device as well.
// constexpr, no HIP call, no ROCm include and of the project aesw_mont.h alone: tests/test_field_headers.py compiles this header
// with g++ and holds it against Python integers.
#pragma once
#include <stdint.h>

#include <utility>

#include "aesw_mont.h"

namespace aesw {

constexpr int FR_LIMBS = MONT_LIMBS;
struct Fr {
    uint32_t l[FR_LIMBS];
};

// r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
constexpr Fr FR_MODULUS = {{0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}};
constexpr Fr FR_ZERO = {{0, 0, 0, 0, 0, 0, 0, 0}};
constexpr uint32_t FR_INV = mont_neg_inverse(FR_MODULUS.l[0]);
static_assert(FR_INV == 0xefffffffu, "-r^-1 mod 2^32");
constexpr Fr FR_RAW_ONE = {{1, 0, 0, 0, 0, 0, 0, 0}};  // mont_mul by it takes a Montgomery form to the plain value
// 2^256 mod r: the Montgomery form of 1
constexpr Fr FR_ONE = {{0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};
template <>
struct MontField<Fr> {
    static constexpr Fr MODULUS = FR_MODULUS, ZERO = FR_ZERO, RAW_ONE = FR_RAW_ONE, ONE = FR_ONE;
    static constexpr uint32_t INV = FR_INV;
};
static_assert(mont_is_canonical(FR_ONE) && mont_eq(mont_mul(FR_ONE, FR_ONE), FR_ONE) && mont_eq(mont_mul(FR_ONE, FR_RAW_ONE), FR_RAW_ONE),
              "R mod r: the Montgomery form of 1 is the identity of mont_mul, and its plain value is 1");

// The core under Fr's names: references to its instantiations, resolved where they are named.  Not functions: a forwarding
// function per name is an inline layer of its own, and changes what hipcc emits for the kernels (profiles/mont_core/README.md).
inline constexpr auto &fr_is_canonical = mont_is_canonical<Fr>;
inline constexpr auto &fr_add = mont_add<Fr>;
inline constexpr auto &fr_sub = mont_sub<Fr>;
inline constexpr auto &fr_mul = mont_mul<Fr>;
inline constexpr auto &fr_is_zero = mont_is_zero<Fr>;
inline constexpr auto &fr_eq = mont_eq<Fr>;

// a^(r - 2): the inverse of a canonical a in Montgomery form (Fermat), and 0 for 0 -- the convention of ff's batch_invert.
// A fixed square-and-multiply over the constant exponent, highest bit first, by loops that stay loops (two products of code; 256
// squarings and one product per set bit of time); the limb of the exponent is chosen among constants, not read from an array.
// One call per batch of a Montgomery inversion (aesw_grand.h), never one per cell.
// Fr's own body, not the core's: it branches on the exponent bit where fq_inv selects, and the kernels that inline it stay as they are.
AESW_MONT_HD constexpr Fr fr_inv(const Fr &a) {
    Fr acc = FR_ONE;
    for (int i = FR_LIMBS - 1; i >= 0; --i) {
        const uint32_t e = mont_inv_exponent_limb<Fr>(i);
        for (int b = 31; b >= 0; --b) {
            acc = mont_mul(acc, acc);
            if (e >> b & 1u) acc = mont_mul(acc, a);
        }
    }
    return acc;
}
// one evaluation at compile time (380 products); fr_inv(0) == 0 and the rest are tests/test_fr_inverse.py's
static_assert(mont_eq(mont_mul(fr_inv(mont_add(FR_ONE, FR_ONE)), mont_add(FR_ONE, FR_ONE)), FR_ONE), "fr_inv(2) * 2 is 1");

// f(i) for i = 0 ... N - 1 with i a constant of the type system (decltype(i)::value): a pack expansion, not a loop.  A loop whose
// body holds field products is too large for the compiler to unroll on request, and a cell array indexed by a loop that
// stays a loop leaves the registers for scratch memory.
template <class F, int... I>
AESW_MONT_HD void fr_each(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
AESW_MONT_HD void fr_unrolled(F &&f) {
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
        acc = mont_add(acc, FR_ONE);
    }
    return t;
}
static_assert(fr_byte_table().cell[0].l[0] == 0 && fr_byte_table().cell[0].l[7] == 0 && fr_byte_table().cell[1].l[0] == FR_ONE.l[0] &&
                  fr_byte_table().cell[1].l[7] == FR_ONE.l[7],
              "cells 0 and 1 are the Montgomery forms of 0 and 1");
static_assert(fr_byte_table().cell[255].l[0] == 0x3ffffabcu && fr_byte_table().cell[255].l[3] == 0x4eace25fu && fr_byte_table().cell[255].l[7] == 0x2fd2eb16u,
              "cell 255 is 255 * 2^256 mod r");

}  // namespace aesw
