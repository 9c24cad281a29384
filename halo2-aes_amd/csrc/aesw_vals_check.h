// aesw_vals_check.h -- MockProver::assert_satisfied for a VALUES witness: the checks of aesw_check.h restated for the layout
// that holds no x column and no y cell of an xor row.  Shared by the device kernel (vals/aesw_vals_check.hip, libaesw_vals.so)
// and the CPU model of the tests (tests/vals_model/), which runs exactly this code.
//
// Every cell VALUES leaves out is the destination of a copy_advice() or a plaintext literal: a host that keeps the reference's
// chips fills it by copying, so the full assignment is determined by the plaintext, the round-key cells of the key slab and the
// 448 y + 608 z bytes.  On that assignment every copy holds by construction and MockProver's criterion for a block reduces to
// its enabled lookups, with every x (and the y of an xor row) RESOLVED through block_copy_graph to the cell it ultimately copies
// from.  The resolution is input independent, like the check table of aesw_check.h.
//
// The VALUES IMAGE of a unit:  y (448) | z (608) | pt (16),  then the PACKED key image  kx | ky | kz | words_column  (the key
// slabs of VALUES are the packed ones).  A root -- the end of a chain of copies -- is a VALUES cell, a plaintext byte or one of
// the 176 round-key cells of round_key_cell(): words_column rows 0..15 and 160 kz cells.
//
// The table has one row entry (aesw_check.h's format: ox | oy << 16,  oz | tag << 16) for each of the 1 056 slab rows whose
// tag is >= 2 -- 160 S-box, 144 mul2, 144 mul3, 608 xor -- in row order, and a parallel array with each entry's slab row.  Rows
// without a lookup (the plaintext rows, the coefficient-1 tmp rows) have nothing to check and no entry.  A block of a values
// witness has no copy checks and no plaintext literal check; key slabs are walked by aesw_check.h's check_key as they are.
#pragma once
#include "aesw_check.h"
#include "aesw_layout.h"  // Geo<VALUES>: the kernel and the CPU model stage a block's y and z by its byte counts

namespace aesw {

constexpr int VALS_ROWS = 1056;                                              // checked rows of a block = VALUES cells of a block
constexpr SlabStrides VALS_ST = slab_strides(VALUES);                        // y, z of a block; the PACKED key slab
constexpr int VALS_O_Z = VALS_ST.y, VALS_O_PT = VALS_O_Z + VALS_ST.z;        // image offsets of z and of the plaintext
constexpr int VALS_BI = VALS_O_PT + 16;                                      // block image bytes: 1 072
constexpr int VALS_KI = VALS_ST.key_bytes();                                 // key image bytes: 936
static_assert(VALS_ROWS == VALS_ST.block_bytes(), "every VALUES cell is the output of one checked row");

// The device form of the table keeps aesw_check.h's word positions, so that check_key and the fast path's key walk read it
// unchanged: the 1 056 row entries at CHK_ROWS, their slab rows behind them (two per word), nothing at CHK_EDGES, and the key
// rows, key edges and gates of the PACKED table at CHK_KROWS / CHK_KEDGES / CHK_GATES with offsets into THIS image.
constexpr int VCHK_SLABROWS = CHK_ROWS + 2 * VALS_ROWS;
static_assert(VCHK_SLABROWS + VALS_ROWS / 2 <= CHK_EDGES, "the slab rows fit behind the row entries");

// words: 2 x VALS_ROWS, rows: VALS_ROWS.  Returns VALS_ROWS, or -1 if a chain of copies ends in a cell the image does not hold
// (it never does: the tests walk every entry).
inline int build_values_check_table(uint32_t *words, uint16_t *rows) {
    uint8_t my[AES_ROWS], mz[AES_ROWS], etag[AES_ROWS];
    int iy[AES_ROWS], iz[AES_ROWS];
    encrypt_values_mask(1, my);
    encrypt_values_mask(2, mz);
    encrypt_selector_tags(etag);
    mask_to_index(my, AES_ROWS, iy);
    mask_to_index(mz, AES_ROWS, iz);
    CopyEdge be[BLOCK_COPIES];
    block_copy_graph(be);
    int from[2][AES_ROWS];  // the edge that writes x / y of a slab row, -1: none
    for (int r = 0; r < AES_ROWS; ++r) from[0][r] = from[1][r] = -1;
    for (int i = 0; i < BLOCK_COPIES; ++i) {
        if (be[i].dst_space != 0 || be[i].dst_col > 1) return -1;
        from[be[i].dst_col][be[i].dst_row] = i;
    }
    const uint32_t kz0 = VALS_BI + VALS_ST.kx + VALS_ST.ky, w0 = kz0 + VALS_ST.kz;
    auto root = [&](uint8_t col, uint16_t row) -> uint32_t {
        CellRef c{0, col, row};
        for (int hops = 0; c.space == 0 && c.col < 2 && from[c.col][c.row] >= 0 && hops < BLOCK_COPIES; ++hops) {
            const CopyEdge &e = be[from[c.col][c.row]];
            c = CellRef{e.src_space, e.src_col, e.src_row};
        }
        if (c.space == 0) {
            if (c.col == 0) return c.row < 16 ? (uint32_t)(VALS_O_PT + c.row) : CHECK_NONE;
            if (c.col == 1) return iy[c.row] >= 0 ? (uint32_t)iy[c.row] : CHECK_NONE;
            return iz[c.row] >= 0 ? (uint32_t)(VALS_O_Z + iz[c.row]) : CHECK_NONE;
        }
        if (c.space == 1) {
            const int i = c.col == 2 ? packed_index_key(2, c.row) : -1;
            return i >= 0 ? kz0 + (uint32_t)i : CHECK_NONE;
        }
        return c.row < 16 ? w0 + c.row : CHECK_NONE;
    };
    int n = 0;
    for (int r = 0; r < AES_ROWS; ++r) {
        if (etag[r] < 2) continue;
        if (n >= VALS_ROWS) return -1;
        const uint32_t ox = root(0, (uint16_t)r);
        uint32_t oy, oz = CHECK_NONE;
        if (etag[r] == 2) {
            oy = root(1, (uint16_t)r);
            oz = iz[r] >= 0 ? (uint32_t)(VALS_O_Z + iz[r]) : CHECK_NONE;
            if (oz == CHECK_NONE) return -1;
        } else {
            oy = iy[r] >= 0 ? (uint32_t)iy[r] : CHECK_NONE;
        }
        if (ox == CHECK_NONE || oy == CHECK_NONE) return -1;
        words[2 * n] = ox | oy << 16;
        words[2 * n + 1] = oz | (uint32_t)etag[r] << 16;
        rows[n] = (uint16_t)r;
        ++n;
    }
    return n == VALS_ROWS ? n : -1;
}

// The device form, CHK_WORDS words.
inline int build_values_device_table(uint32_t *t) {
    for (int i = 0; i < CHK_WORDS; ++i) t[i] = 0;
    uint16_t rows[VALS_ROWS];
    if (build_values_check_table(t + CHK_ROWS, rows) != VALS_ROWS) return -1;
    for (int e = 0; e < VALS_ROWS; ++e) t[VCHK_SLABROWS + e / 2] |= (uint32_t)rows[e] << (16 * (e & 1));
    uint32_t packed[CHK_WORDS];
    build_check_table(PACKED, packed);
    const uint32_t shift = check_geo(PACKED).bi - VALS_BI;  // the key image starts behind a smaller block image here
    auto rebase = [&](uint32_t o) { return o == CHECK_NONE ? o : o - shift; };
    for (int r = 0; r < KEY_ROWS; ++r) {
        const uint32_t a = packed[CHK_KROWS + 2 * r], b = packed[CHK_KROWS + 2 * r + 1];
        t[CHK_KROWS + 2 * r] = rebase(a & 0xffffu) | rebase(a >> 16) << 16;
        t[CHK_KROWS + 2 * r + 1] = rebase(b & 0xffffu) | (b & 0xffff0000u);
    }
    for (int i = 0; i < KEY_COPIES; ++i) {
        const uint32_t d = packed[CHK_KEDGES + i];
        t[CHK_KEDGES + i] = rebase(d & 0xffffu) | rebase(d >> 16) << 16;
    }
    for (int r = 0; r < WORDS_ROWS; ++r) {
        const uint32_t g = packed[CHK_GATES + r];
        t[CHK_GATES + r] = rebase(g & 0xffffu) | (g & 0xffff0000u);
    }
    return 0;
}

AESW_HD uint32_t values_slab_row(const uint32_t *t, uint32_t e) { return (t[VCHK_SLABROWS + e / 2] >> (16 * (e & 1))) & 0xffffu; }

// The checks of one block of a values witness (lanes lane, lane + nlanes, ...): the exact, counting walk, with the failure
// keys of check_block.  t: the device form of the table; ct: the block's 16 output bytes, or null.
AESW_HD void check_values_block(const uint8_t *img, const uint32_t *t, const uint8_t *tab768, const uint8_t *ct, uint64_t unit, uint32_t lane,
                                uint32_t nlanes, CheckAcc &acc) {
    for (uint32_t e = lane; e < (uint32_t)VALS_ROWS; e += nlanes)
        if (!check_row_ok(img, tab768, t[CHK_ROWS + 2 * e], t[CHK_ROWS + 2 * e + 1])) acc.hit(CHK_LOOKUP, unit, 0, values_slab_row(t, e));
    if (ct)  // the last sixteen entries are slab rows 1344..1359: their z cells are the ciphertext
        for (uint32_t i = lane; i < 16; i += nlanes)
            if (img[t[CHK_ROWS + 2 * (VALS_ROWS - 16 + i) + 1] & 0xffffu] != ct[i]) acc.hit(CHK_INPUT, unit, 0, AES_ROWS - 16 + i);
}

}  // namespace aesw
