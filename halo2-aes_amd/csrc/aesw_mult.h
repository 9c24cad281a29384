// aesw_mult.h -- the bin rule of the lookup multiplicities, once: which row of the lookup table (aesw_lookup_table,
// src/table.rs:18-192) the INPUT operands of an enabled lookup name, and whether the lookup is a hit, i.e. that row really
// holds the lookup's output.  One source for the kernels of libaesw_mult.so and libaesw_acc.so (through
// aesw_mult_dev.h), the pure-host aesw_mult_bin and the CPU test of the rule; with it the sizes of the LDS counter split and
// what the entry points of both libraries accept.  The tag of a row is enc_row_tag / key_row_tag's (aesw_slabmap.h) and the
// set a block lies in is Placement's (aesw_placement.h): neither is restated here.
// No HIP call and no ROCm include: tests/test_mult_rule.py compiles this header alone with g++.
//
// The table has five sections, in the order load_enc_full_table() writes them, and one all-zero row behind them:
//   tag 1 U8      rows     0 ..    255   (1, x, 0, 0)                 bin = x                  hit: always
//   tag 3 Sbox    rows   256 ..    511   (3, x, sbox[x], 0)           bin = 256 + x            hit: y == sbox[x]
//   tag 2 Xor     rows   512 .. 66 047   (2, x, y, x ^ y)             bin = 512 + 256 x + y    hit: z == x ^ y
//   tag 4 GfMul2  rows 66 048 .. 66 303  (4, x, mul2[x], 0)           bin = 66 048 + x         hit: y == mul2[x]
//   tag 5 GfMul3  rows 66 304 .. 66 559  (5, x, mul3[x], 0)           bin = 66 304 + x         hit: y == mul3[x]
//                 row  66 560            (0, 0, 0, 0)                 never counted
// A lookup that is not a hit has no table row: it is counted in no bin, as a miss.  A row without a lookup (tag 0) and the rows
// of a set that no block fills are "disabled": the prover's compressed input there is the all-zero row, which a histogram
// leaves at 0.  A host that needs it takes it per ARGUMENT, not per set: for the argument (set s, tag t) over 2^k rows,
//   multiplicity of the zero row = 2^k - (the sum of section t of set s's histogram)        [with no miss in the set]
// since every row of the set is either an enabled lookup of tag t, counted in section t, or compresses to the zero row.
#pragma once
#include "../../include/aesw.h"
#include "aesw_slabmap.h"

namespace aesw {

constexpr uint32_t MULT_BINS = 66561;      // rows of the table = bins of one histogram
constexpr uint32_t MULT_ZERO_ROW = 66560;  // always 0
constexpr uint32_t MULT_NO_BIN = ~0u;      // tag 0, or no tag at all
static_assert(MULT_BINS == AESW_TABLE_ROWS, "one bin per table row");

// first row and row count of the section of a tag (0 rows for tag 0 and for anything that is no tag)
AESW_HD constexpr uint32_t mult_section_first(uint32_t tag) {
    return tag == 1 ? 0u : tag == 3 ? 256u : tag == 2 ? 512u : tag == 4 ? 66048u : tag == 5 ? 66304u : MULT_ZERO_ROW;
}
AESW_HD constexpr uint32_t mult_section_rows(uint32_t tag) { return tag == 2 ? 65536u : (tag >= 1 && tag <= 5) ? 256u : 0u; }
static_assert(mult_section_first(3) == mult_section_first(1) + mult_section_rows(1) && mult_section_first(2) == mult_section_first(3) + mult_section_rows(3) &&
              mult_section_first(4) == mult_section_first(2) + mult_section_rows(2) && mult_section_first(5) == mult_section_first(4) + mult_section_rows(4) &&
              MULT_ZERO_ROW == mult_section_first(5) + mult_section_rows(5), "the sections tile the table in load_enc_full_table()'s order");

// The bin of a lookup: x, y are bytes (only their low eight bits are read).
AESW_HD constexpr uint32_t mult_bin(uint32_t tag, uint32_t x, uint32_t y) {
    return (tag < 1 || tag > 5) ? MULT_NO_BIN : mult_section_first(tag) + (tag == 2 ? (x & 0xffu) << 8 | (y & 0xffu) : (x & 0xffu));
}
// Is (tag, x, y, z) a row of the table built from tab768 = sbox | mul2 | mul3 (the context's runtime tables)?  A U8 row keeps
// no y and no z cell: whatever is passed for them is ignored, as z is for the three one-operand tags.
AESW_HD constexpr bool mult_hit(uint32_t tag, uint32_t x, uint32_t y, uint32_t z, const uint8_t *tab768) {
    const bool one_operand = tag >= 3 && tag <= 5;
    const uint32_t lk = tab768[(one_operand ? tag - 3 : 0u) * 256 + (x & 0xffu)];  // one load whatever the tag: no branch in a kernel
    return tag == 1 || (tag == 2 ? z == (x ^ y) : one_operand && y == lk);
}

// The counter split of the kernels that count in LDS.  A full histogram does not fit the LDS of a workgroup, so a unit goes to
// a PAIR of workgroups, both of which see every row.  half 0 owns the Xor bins with x < 128 (rows 512 .. 33 279) and the four
// small sections, half 1 the Xor bins with x >= 128 (rows 33 280 .. 66 047); each keeps MULT_COUNTERS counters: the XOR_HALF of
// its Xor half, then -- used by half 0 alone -- the SMALL ones, U8 | Sbox | GfMul2 | GfMul3 as 1 024 consecutive counters.
constexpr uint32_t XOR_FIRST = mult_section_first(2), XOR_HALF = mult_section_rows(2) / 2, SMALL = 4 * 256, SMALL_LOW = 2 * 256;
constexpr uint32_t MULT_COUNTERS = XOR_HALF + SMALL;
static_assert(XOR_FIRST == SMALL_LOW && mult_section_first(4) == XOR_FIRST + 2 * XOR_HALF && MULT_ZERO_ROW == mult_section_first(4) + SMALL_LOW,
              "two small sections in front of the Xor section, two behind it");
// Where `half` counts a hit of tag 1 ... 5 on the bytes x, y: does it own the bin, and which of its counters is the bin's
// (LdsSink::add of aesw_mult_dev.h, expression for expression).
AESW_HD constexpr bool mult_half_owns(uint32_t half, uint32_t tag, uint32_t x) { return tag == 2 ? ((x & 0xffu) >> 7) == half : half == 0; }
AESW_HD constexpr uint32_t mult_counter(uint32_t half, uint32_t tag, uint32_t x, uint32_t y) {
    return tag == 2 ? mult_bin(tag, x, y) - XOR_FIRST - half * XOR_HALF
                    : XOR_HALF + (mult_bin(tag, x, y) < XOR_FIRST ? mult_bin(tag, x, y) : mult_bin(tag, x, y) - 2 * XOR_HALF);
}
// What a half flushes: counters [counter, counter + length) are bins [bin, bin + length).  Range 0 is the Xor half; half 0
// has ranges 1 and 2 as well, the small sections in front of the Xor section and behind it.
struct MultFlushRange {
    uint32_t bin, counter, length;
};
AESW_HD constexpr uint32_t mult_flush_ranges(uint32_t half) { return half == 0 ? 3u : 1u; }
AESW_HD constexpr MultFlushRange mult_flush_range(uint32_t half, uint32_t i) {
    return i == 0   ? MultFlushRange{XOR_FIRST + half * XOR_HALF, 0u, XOR_HALF}
           : i == 1 ? MultFlushRange{0u, XOR_HALF, SMALL_LOW}
                    : MultFlushRange{XOR_FIRST + 2 * XOR_HALF, XOR_HALF + SMALL_LOW, SMALL_LOW};
}

// What the entry points accept.  A histogram counts rows of one set, and a set has 2^k rows: with k <= MULT_MAX_K every count
// fits the 32 bits of a bin (and of an LDS counter), identical blocks included.
constexpr uint32_t MULT_MIN_K = 2, MULT_MAX_K = 30, MULT_MAX_SETS = 1024;
static_assert(MULT_MAX_K < 32, "a bin holds 2^k");
AESW_HD constexpr bool mult_k_ok(uint32_t k) { return k >= MULT_MIN_K && k <= MULT_MAX_K; }
AESW_HD constexpr bool mult_sets_ok(uint32_t n_sets) { return n_sets >= 1 && n_sets <= MULT_MAX_SETS; }
// a circuit of fewer than KEY_ROWS rows has no room for the key schedule: no key selector is enabled there
// (aesw_assemble_selectors)
AESW_HD constexpr bool mult_has_key_rows(uint32_t k) { return ((uint64_t)1 << k) >= KEY_ROWS; }

// Enabled lookups of one block slab / one key slab, per tag: counted off the classifiers.
constexpr uint32_t mult_block_lookups(uint32_t tag) {
    uint32_t n = 0;
    for (int r = 0; r < AES_ROWS; ++r) n += (uint32_t)enc_row_tag(r) == tag;
    return n;
}
constexpr uint32_t mult_key_lookups(uint32_t tag) {
    uint32_t n = 0;
    for (int r = 0; r < KEY_ROWS; ++r) n += (uint32_t)key_row_tag(r) == tag;
    return n;
}
constexpr uint32_t MULT_BLOCK_LOOKUPS = AES_ROWS - mult_block_lookups(0), MULT_KEY_LOOKUPS = KEY_ROWS - mult_key_lookups(0);
static_assert(MULT_BLOCK_LOOKUPS == 1056 && mult_block_lookups(1) == 0 && mult_block_lookups(2) == 608 && mult_block_lookups(3) == 160 &&
              mult_block_lookups(4) == 144 && mult_block_lookups(5) == 144, "a block: 608 Xor, 160 Sbox, 144 GfMul2, 144 GfMul3; 304 rows are plain copies");
static_assert(MULT_KEY_LOOKUPS == 400 && mult_key_lookups(1) == 160 && mult_key_lookups(2) == 200 && mult_key_lookups(3) == 40, "a key slab: 160 U8, 200 Xor, 40 Sbox");

}  // namespace aesw
