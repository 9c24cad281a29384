// aesw_vacc.h -- the image and the table of libaesw_vacc.so (vacc/aesw_vacc.hip): the lookup multiplicities of a
// VALUES witness.  The lookups of a block and where their operands lie are aesw_vals_check.h's (build_values_check_table): a
// VALUES cell, a plaintext byte or one of the 176 round-key cells, which sit in kz and in words_column of the PACKED key slab.
// A counting wave needs of the key slab those two columns alone, so ITS image drops kx and ky:
//     aesw_vals.h's image   y (448) | z (608) | pt (16) | kx (400) | ky (240) | kz (200) | words_column (96)     2 008 bytes
//     the image here        y (448) | z (608) | pt (16) | kz (200) | words_column (96)                           1 368 bytes
// and every offset behind the block image moves down by kx + ky, once, when the table is built.  The table: the 1 056 row entries
// in aesw_check.h's format (ox | oy << 16, oz | tag << 16), then their slab rows, two per word.
// Pure host code, no HIP call and no ROCm include: tests/test_vacc_model.py compiles this header alone with g++.
#pragma once
#include "aesw_vals_check.h"

namespace aesw {

constexpr int VACC_KEY_DROP = VALS_ST.kx + VALS_ST.ky;                      // 640: the key columns no lookup of a block reads
constexpr int VACC_O_KZ = VALS_BI, VACC_O_W = VACC_O_KZ + VALS_ST.kz;       // 1 072, 1 272
constexpr int VACC_BI = VACC_O_W + WORDS_ROWS;                              // 1 368 bytes hold every operand
constexpr int VACC_IMG = (VACC_BI + 15) / 16 * 16;                          // a wave's image: the next one starts 16-byte aligned
constexpr int VACC_SLABROWS = 2 * VALS_ROWS, VACC_WORDS = VACC_SLABROWS + VALS_ROWS / 2;
static_assert(VALS_ROWS % 2 == 0 && VACC_O_KZ % 16 == 0 && VACC_O_W % 8 == 0 && VALS_ST.kz % 8 == 0 && WORDS_ROWS % 8 == 0, "kz and words_column travel as 8-byte units");
static_assert(VALS_KI == VACC_KEY_DROP + VALS_ST.kz + WORDS_ROWS, "the packed key image is kx | ky | kz | words_column");

// An offset of aesw_vals.h's image as an offset of the image here; CHECK_NONE stays.  A block's lookups read no kx and no ky
// cell: such an offset has no place here and becomes CHECK_NONE, which build_vacc_table refuses.
constexpr uint32_t vacc_rebase(uint32_t o) {
    return o == CHECK_NONE || o < (uint32_t)VALS_BI ? o : o < (uint32_t)(VALS_BI + VACC_KEY_DROP) ? CHECK_NONE : o - (uint32_t)VACC_KEY_DROP;
}
static_assert(vacc_rebase(0) == 0 && vacc_rebase(VALS_BI - 1) == VALS_BI - 1 && vacc_rebase(VALS_BI + VACC_KEY_DROP) == VACC_O_KZ &&
              vacc_rebase(VALS_BI + VALS_KI - 1) == VACC_BI - 1 && vacc_rebase(VALS_BI) == CHECK_NONE && vacc_rebase(CHECK_NONE) == CHECK_NONE, "y | z | pt stay, kz | words move down");

// VACC_WORDS words.  Returns 0, or -1 if the table of aesw_vals_check.h cannot be built or an operand lies in kx or ky.
inline int build_vacc_table(uint32_t *t) {
    uint16_t rows[VALS_ROWS];
    for (int i = 0; i < VACC_WORDS; ++i) t[i] = 0;
    if (build_values_check_table(t, rows) != VALS_ROWS) return -1;
    for (int e = 0; e < VALS_ROWS; ++e) {
        const uint32_t a = t[2 * e], b = t[2 * e + 1];
        const uint32_t ox = vacc_rebase(a & 0xffffu), oy = vacc_rebase(a >> 16), oz = vacc_rebase(b & 0xffffu), tag = b >> 16;
        if (ox == CHECK_NONE || oy == CHECK_NONE || (tag == 2 && oz == CHECK_NONE)) return -1;
        if (e && rows[e] <= rows[e - 1]) return -1;  // row order: the smallest entry with a miss is the smallest slab row with one
        t[2 * e] = ox | oy << 16;
        t[2 * e + 1] = oz | tag << 16;
        t[VACC_SLABROWS + e / 2] |= (uint32_t)rows[e] << (16 * (e & 1));
    }
    return 0;
}
AESW_HD uint32_t vacc_slab_row(const uint32_t *t, uint32_t e) { return (t[VACC_SLABROWS + e / 2] >> (16 * (e & 1))) & 0xffffu; }

}  // namespace aesw
