// aesw_theta.h -- the rules of libaesw_theta.so, once: which of the three compressed tables an argument reads,
// what a row of the table compresses to under theta, which table row stands at a row of the circuit's table column, and which
// table row the compressed INPUT of an argument is at a row of the circuit.  One source for the kernels of theta/aesw_theta.hip
// and the CPU test of the rules.  Nothing is restated: the sections and the bin and hit rule are aesw_mult.h's, the tag of a
// row and the packed indices aesw_slabmap.h's, where a circuit puts a block and which byte a cell holds aesw_placement.h's
// (column_source / block_byte / key_byte), the kind of a miss aesw_check.h's, the field aesw_fr.h's.
// No HIP call and no ROCm include: tests/test_theta_model.py compiles this header alone with g++.
#pragma once
#include "aesw_check.h"
#include "aesw_fr.h"
#include "aesw_mult.h"
#include "aesw_placement.h"

namespace aesw {

constexpr uint32_t THETA_TABLES = 3, THETA_TAGS = 5;
constexpr uint32_t THETA_MISS = ~0u;  // the input cell of an enabled lookup that names no table row

// The chips fix how many expressions an argument compresses: the tag and 1, 2 or 3 operands.  Table j has arity j + 2.
AESW_HD constexpr uint32_t theta_table_of_tag(uint32_t tag) { return tag == 1 ? 0u : tag == 2 ? 2u : 1u; }
AESW_HD constexpr uint32_t theta_arity(uint32_t table) { return table + 2; }

// The four bytes of table row r < MULT_BINS as load_enc_full_table() writes them, from the runtime tables tab768 = sbox | mul2 |
// mul3: the inverse of mult_bin inside the section r lies in, and the output mult_hit accepts there.
struct ThetaTableRow {
    uint32_t tag, a, b, c;
};
AESW_HD constexpr uint32_t theta_section_tag(uint32_t r) {
    uint32_t tag = 0;
    for (uint32_t t = 1; t <= THETA_TAGS; ++t)
        if (r - mult_section_first(t) < mult_section_rows(t)) tag = t;  // unsigned: r below the section wraps
    return tag;
}
AESW_HD constexpr ThetaTableRow theta_table_row(uint32_t r, const uint8_t *tab768) {
    const uint32_t tag = theta_section_tag(r);
    if (tag == 0) return ThetaTableRow{0, 0, 0, 0};  // MULT_ZERO_ROW
    const uint32_t o = r - mult_section_first(tag);
    if (tag == 2) return ThetaTableRow{tag, o >> 8, o & 0xffu, (o >> 8) ^ (o & 0xffu)};
    return ThetaTableRow{tag, o, tag == 1 ? 0u : (uint32_t)tab768[(tag - 3) * 256 + o], 0};
}

// halo2's compression: acc = acc * theta + e over the first `arity` (2, 3 or 4) of the expressions tag, a, b, c, given as the
// Montgomery forms of the four bytes; theta canonical.
AESW_MONT_HD constexpr Fr theta_compress(const Fr &theta, const Fr &tag, const Fr &a, const Fr &b, const Fr &c, uint32_t arity) {
    Fr acc = fr_add(fr_mul(tag, theta), a);
    if (arity >= 3) acc = fr_add(fr_mul(acc, theta), b);
    if (arity >= 4) acc = fr_add(fr_mul(acc, theta), c);
    return acc;
}

// The table column in row order: the 66 561 rows, pad_row behind them.
AESW_HD constexpr uint32_t theta_table_index(uint32_t i, uint32_t pad_row) { return i < MULT_BINS ? i : pad_row; }

// What stands at one row of one set, resolved once for the set's five arguments: the row's tag (0: every argument reads the
// all-zero row there) and the cell of the argument of that tag -- the bin, or THETA_MISS -- with the key of a miss in the
// encoding of aesw_mult_report.first_miss.
struct ThetaInput {
    uint32_t tag, cell;
    uint64_t miss_key;
};
// cs[c]: column_source of the set's column c = x, y, z; with_keys: set 0 holds a key slab and 2^k rows hold the key rows.
AESW_HD ThetaInput theta_input_row(const ColumnSource cs[3], int packed, bool with_keys, uint32_t row, uint64_t n_blocks, const uint8_t *tab768) {
    ThetaInput in{0, MULT_ZERO_ROW, ~0ull};
    const uint32_t base = cs[0].base;
    uint32_t x = 0, y = 0, z = 0, r = row, is_key = 0;
    uint64_t unit = 0;
    if (row < base) {
        if (!with_keys) return in;
        in.tag = (uint32_t)key_row_tag((int)row);
        is_key = 1;
        x = key_byte(cs[0], packed, row); y = key_byte(cs[1], packed, row); z = key_byte(cs[2], packed, row);
    } else {
        const uint32_t rr = row - base, bi = rr / (uint32_t)AES_ROWS;
        r = rr - bi * (uint32_t)AES_ROWS;
        if (bi >= cs[0].cap || cs[0].b0 + bi >= n_blocks) return in;
        in.tag = (uint32_t)enc_row_tag((int)r);
        unit = cs[0].b0 + bi;
        x = block_byte(cs[0], packed, bi, r, n_blocks); y = block_byte(cs[1], packed, bi, r, n_blocks); z = block_byte(cs[2], packed, bi, r, n_blocks);
    }
    if (in.tag == 0) return in;
    if (mult_hit(in.tag, x, y, z, tab768)) {
        in.cell = mult_bin(in.tag, x, y);
    } else {
        in.cell = THETA_MISS;
        in.miss_key = unit << 20 | (uint64_t)(is_key << 19 | (uint32_t)CHK_LOOKUP << 16 | r);
    }
    return in;
}

}  // namespace aesw
