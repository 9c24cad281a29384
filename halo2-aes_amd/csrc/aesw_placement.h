// aesw_placement.h -- where a circuit puts its blocks, described once for the host entry points (aesw_api.cpp), the assemble
// kernels (aesw_kernels.hip) and the column checker (cols/aesw_cols_check.hip); DESIGN.md "The placement rule".
// FixedAes128Config::aes_callable, src/aes128.rs:303-325, restated: set 0 is charged KEY_SCHEDULE_ROWS of its 2^K rows, every
// set holds whole AES_ROWS-row blocks, set 0's blocks start behind the KEY_ROWS rows the key schedule really uses, and
// words_column is the last column.  No HIP call and no ROCm include: tests/test_placement.py compiles this header alone with
// g++ and holds it against the reference's rule, restated there a second time, and against the oracle's circuit.
#pragma once
#include "../../include/aesw.h"
#include "aesw_slabmap.h"

namespace aesw {

// Blocks per column set.  A kernel parameter block embeds one, filled by its launcher, so that no kernel divides for it.
struct Placement {
    uint64_t cap0, capn;  // set 0 / every other set
    Placement() = default;
    AESW_HD explicit Placement(uint32_t k)  // k <= 40 on the host, <= 30 wherever a kernel works in 32 bits
        : cap0(((uint64_t)1 << k) >= AESW_KEY_SCHEDULE_ROWS ? (((uint64_t)1 << k) - AESW_KEY_SCHEDULE_ROWS) / AES_ROWS : 0),
          capn(((uint64_t)1 << k) / AES_ROWS) {}
    AESW_HD uint64_t capacity(uint32_t set) const { return set == 0 ? cap0 : capn; }
    AESW_HD uint64_t total(uint32_t n_sets) const { return n_sets == 0 ? 0 : cap0 + (uint64_t)(n_sets - 1) * capn; }  // aesw_block_capacity
    AESW_HD uint64_t first_block(uint32_t set) const { return set == 0 ? 0 : cap0 + (uint64_t)(set - 1) * capn; }    // circuit-local
    AESW_HD static uint32_t first_row(uint32_t set) { return set == 0 ? KEY_ROWS : 0; }
    // Block j of a circuit (j < total(n_sets): the caller has checked) -> its set and its index there.  T is the width of the
    // division: uint64_t on the host, uint32_t where an entry point has bounded j (the checker, K <= 30).
    template <class T>
    AESW_HD void locate(uint64_t j, uint32_t &set, T &bi) const {
        set = 0;
        bi = (T)j;
        if (j >= cap0) {
            const T jj = (T)(j - cap0), cn = (T)capn;
            set = 1 + (uint32_t)(jj / cn);
            bi = jj - (T)(set - 1) * cn;
        }
    }
    AESW_HD static uint64_t row_of(uint32_t set, uint64_t bi) { return first_row(set) + bi * AES_ROWS; }
    // blocks of set `set` that a circuit of n_c blocks fills
    AESW_HD uint64_t filled(uint32_t set, uint64_t n_c) const {
        const uint64_t cap_s = capacity(set), b0 = first_block(set);
        return n_c > b0 ? (n_c - b0 < cap_s ? n_c - b0 : cap_s) : 0;
    }
};

// What a cell's source depends on through its column alone (scalar in a kernel whose workgroup writes one column).
struct ColumnSource {
    bool words;          // words_column: the last one
    uint32_t set, c;     // column set, and 0 / 1 / 2 = x / y / z in it
    uint32_t base;       // first_row(set); 0 for words_column
    uint64_t cap, b0;    // capacity(set), first_block(set)
    const uint8_t *kc;   // the key slab's column c (may be null)
    const uint8_t *sc;   // the block slabs' column c ...
    uint32_t stride;     // ... and its bytes per block
};

AESW_HD ColumnSource column_source(const Placement &pl, uint32_t col, uint32_t n_sets, const uint8_t *kx, const uint8_t *ky, const uint8_t *kz,
                                   const uint8_t *x, const uint8_t *y, const uint8_t *z, uint32_t sx, uint32_t sy, uint32_t sz) {
    ColumnSource s;
    s.words = col == 3 * n_sets;
    s.set = col / 3;
    s.c = col - 3 * s.set;
    s.base = (!s.words && s.set == 0) ? KEY_ROWS : 0;
    s.kc = s.c == 0 ? kx : s.c == 1 ? ky : kz;
    s.sc = s.c == 0 ? x : s.c == 1 ? y : z;
    s.stride = s.c == 0 ? sx : s.c == 1 ? sy : sz;
    s.cap = pl.capacity(s.set);
    s.b0 = pl.first_block(s.set);
    return s;
}

// The byte synthesize() puts at one row of that column, 0 where nothing is ever assigned: a words_column row, a key row
// (row < base) or row r of the set's block bi.  cell_byte() splits a row into the three; a kernel whose grid has split it
// already calls the part.  n_blocks: the blocks the circuit holds; `packed`: the slabs are PACKED, not DENSE.
AESW_HD uint32_t words_byte(const uint8_t *kw, uint64_t row) { return (row < WORDS_ROWS && kw) ? kw[row] : 0u; }
AESW_HD uint32_t key_byte(const ColumnSource &s, int packed, uint32_t row) {
    const int idx = packed ? packed_index_key((int)s.c, (int)row) : (int)row;
    return (s.kc && idx >= 0) ? s.kc[idx] : 0u;
}
AESW_HD uint32_t block_byte(const ColumnSource &s, int packed, uint64_t bi, uint32_t r, uint64_t n_blocks) {
    const int idx = packed ? packed_index_enc((int)s.c, (int)r) : (int)r;
    return (bi < s.cap && s.b0 + bi < n_blocks && idx >= 0) ? s.sc[(s.b0 + bi) * s.stride + idx] : 0u;
}
template <class R>  // the width of the row and of its division by AES_ROWS: uint32_t for K <= 30, uint64_t for any K
AESW_HD uint32_t cell_byte(const ColumnSource &s, const uint8_t *kw, int packed, R row, uint64_t n_blocks) {
    if (s.words) return words_byte(kw, row);
    if (row < s.base) return key_byte(s, packed, (uint32_t)row);
    const R rr = row - s.base, bi = rr / AES_ROWS;
    return block_byte(s, packed, bi, (uint32_t)(rr - bi * AES_ROWS), n_blocks);
}

}  // namespace aesw
