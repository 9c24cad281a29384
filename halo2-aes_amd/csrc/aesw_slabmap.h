// aesw_slabmap.h -- the slab map, once: which rows a block slab and a key slab have, which chip is enabled on each, and which
// of its x / y / z cells are assigned (DESIGN.md 2 gives it as a table; "The slab map" in 4.4 says who reads this header).
// Two classifiers walk the reference's region call order (src/aes128.rs:154-301, src/key_schedule.rs:80-224) and say a row's
// tag; one rule says which cells a tag assigns and which a layout keeps; the masks, the tag arrays, the strides of the seven
// columns, the packed indices and the copy counts are all derived from those by counting, and checked here at compile time.
// Nothing is copied from the reference: the numbers are rows and byte offsets of OUR column-major buffers.
// No HIP call and no ROCm include: tests/test_slabmap.py compiles this header alone with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AESW_HD __host__ __device__ __forceinline__
#else
#define AESW_HD inline
#endif

namespace aesw {

// DENSE: exact image of the advice rows.  PACKED: assigned cells only, row order.  VALUES: only the cells
// whose value a chip's closure computes -- y of the S-box and mul rows, z of the xor rows; column x and the
// y cells of xor rows are copy_advice() of earlier cells in the reference (src/chips/*.rs) and are omitted.
enum : int { DENSE = 0, PACKED = 1, VALUES = 2 };

constexpr int AES_ROWS = 1360;  // src/constant.rs:114
constexpr int KEY_ROWS = 400;   // 10 rounds x 40 one-row chip regions (src/key_schedule.rs:122-224)
constexpr int WORDS_ROWS = 96;  // 16 + 10 x (4 + 4) rows of words_column
constexpr int RK_BYTES = 176;   // 11 round keys

// MixColumns matrix rows as the reference writes them (src/aes128.rs:228-233).
constexpr int MIX[4][4] = {{2, 3, 1, 1}, {1, 2, 3, 1}, {1, 1, 2, 3}, {3, 1, 1, 2}};

// ---- the two row classifiers ----------------------------------------------------------------------------------------
// The chip whose selector is enabled on a row, as the Tag of its lookup (src/table.rs:10-16): 0 none (plain copy / assign
// regions), 1 U8 range, 2 Xor, 3 Sbox, 4 GfMul2, 5 GfMul3.

// Block slab: 16 plaintext rows, the initial AddRoundKey (src/aes128.rs:176-198), rounds 1..9 of 144 rows at 32 + 144 (R - 1)
// -- 16 S-box rows, 16 lcon() records of 7 rows at 16 + 7 k (four products of MIX row k & 3, three xors), 16 AddRoundKey
// rows (:201-262) -- and round 10: 16 S-box rows, then ShiftRows ^ rk10.
AESW_HD constexpr int enc_row_tag(int r) {
    if (r < 16) return 0;
    if (r < 32) return 2;
    if (r >= 1328) return r < 1344 ? 3 : 2;
    const int q = (r - 32) % 144;
    if (q < 16) return 3;
    if (q >= 128) return 2;
    const int k = (q - 16) / 7, t = (q - 16) % 7;
    if (t >= 4) return 2;
    return MIX[k & 3][t] == 1 ? 0 : MIX[k & 3][t] == 2 ? 4 : 5;
}

// Key slab: round rho at 40 rho -- 4 S-box rows, 20 xor rows (rcon, then the four words), 16 range rows.
AESW_HD constexpr int key_row_tag(int r) {
    const int j = r % 40;
    return j < 4 ? 3 : j < 24 ? 2 : 1;
}

// words_column: q_eq_rcon is enabled on row 20 + 8 rho, where the fixed column holds the round constant
// (src/key_schedule.rs:161-175); 0 elsewhere.
struct WordsRow { uint8_t q_eq_rcon, rcon; };
AESW_HD constexpr WordsRow words_row(int r) {
    constexpr uint8_t RC[10] = {1, 2, 4, 8, 16, 32, 64, 128, 27, 54};
    return r >= 20 && (r - 20) % 8 == 0 ? WordsRow{1, RC[(r - 20) / 8]} : WordsRow{0, 0};
}

// ---- the cell rule, on a tag ----------------------------------------------------------------------------------------
// In both slabs x is always assigned, y iff the row has a lookup with an input pair (tag >= 2), z iff it is an xor row.
AESW_HD constexpr bool cell_assigned(int col, int tag) { return col == 0 || (col == 1 ? tag >= 2 : tag == 2); }
// DENSE keeps every row, PACKED the assigned cells, VALUES the cells a closure computes: y of a table row, z of an xor row.
AESW_HD constexpr bool cell_kept(int layout, int col, int tag) {
    return layout == DENSE || (layout == PACKED ? cell_assigned(col, tag) : col == 1 ? tag >= 3 : col == 2 && tag == 2);
}
// VALUES keeps the PACKED key slab (one key slab per circuit in the reference's call shape; nothing to save there)
AESW_HD constexpr int key_slab_layout(int layout) { return layout == DENSE ? DENSE : PACKED; }

// ---- everything derived ---------------------------------------------------------------------------------------------
// Pure host: which dense rows of the encrypt slab are assigned, per column; the tests compare it with the mask the oracle
// derives by running the reference's call order.
constexpr void encrypt_assigned_mask(int col, uint8_t mask[AES_ROWS]) {
    for (int r = 0; r < AES_ROWS; ++r) mask[r] = cell_assigned(col, enc_row_tag(r));
}
// ... that the VALUES layout keeps (col 1: y of S-box / mul rows, col 2: z of xor rows; col 0: none), in row order
constexpr void encrypt_values_mask(int col, uint8_t mask[AES_ROWS]) {
    for (int r = 0; r < AES_ROWS; ++r) mask[r] = cell_kept(VALUES, col, enc_row_tag(r));
}
constexpr void key_assigned_mask(int col, uint8_t mask[KEY_ROWS]) {
    for (int r = 0; r < KEY_ROWS; ++r) mask[r] = cell_assigned(col, key_row_tag(r));
}
// Fixed data for keygen: the tag of every slab row, and words_column's gate.
constexpr void encrypt_selector_tags(uint8_t tag[AES_ROWS]) {
    for (int r = 0; r < AES_ROWS; ++r) tag[r] = (uint8_t)enc_row_tag(r);
}
constexpr void key_selector_tags(uint8_t tag[KEY_ROWS], uint8_t q_eq_rcon[WORDS_ROWS], uint8_t rcon_fixed[WORDS_ROWS]) {
    for (int r = 0; r < KEY_ROWS; ++r) tag[r] = (uint8_t)key_row_tag(r);
    for (int r = 0; r < WORDS_ROWS; ++r) { q_eq_rcon[r] = words_row(r).q_eq_rcon; rcon_fixed[r] = words_row(r).rcon; }
}

// The index of a kept row among the kept rows -- the prefix count of its mask --, -1 for a row that is left out.  Returns the count.
template <class I>
constexpr int mask_to_index(const uint8_t *mask, int n, I *idx) {
    int kept = 0;
    for (int r = 0; r < n; ++r) idx[r] = mask[r] ? kept++ : -1;
    return kept;
}

// The seven columns of a batch in their fixed order -- x, y, z of a block, words_column and kx, ky, kz of a key -- and the
// bytes one unit takes in each: the number of cells the layout keeps.
struct SlabStrides {
    uint32_t x, y, z, words, kx, ky, kz;
    AESW_HD constexpr uint32_t operator[](int c) const {
        const uint32_t v[7] = {x, y, z, words, kx, ky, kz};
        return v[c];
    }
    AESW_HD constexpr uint32_t block_bytes() const { return x + y + z; }           // a block's image  x | y | z
    AESW_HD constexpr uint32_t key_bytes() const { return kx + ky + kz + words; }  // a key's image  kx | ky | kz | words_column
};
constexpr SlabStrides count_slab_strides(int layout) {
    SlabStrides s{0, 0, 0, WORDS_ROWS, 0, 0, 0};
    for (int r = 0; r < AES_ROWS; ++r) {
        const int t = enc_row_tag(r);
        s.x += cell_kept(layout, 0, t); s.y += cell_kept(layout, 1, t); s.z += cell_kept(layout, 2, t);
    }
    for (int r = 0; r < KEY_ROWS; ++r) {
        const int t = key_row_tag(r), kl = key_slab_layout(layout);
        s.kx += cell_kept(kl, 0, t); s.ky += cell_kept(kl, 1, t); s.kz += cell_kept(kl, 2, t);
    }
    return s;
}
constexpr SlabStrides SLAB_STRIDES[3] = {count_slab_strides(DENSE), count_slab_strides(PACKED), count_slab_strides(VALUES)};
// all zero for a layout that is none of the three, like the public aesw_column_stride
AESW_HD constexpr SlabStrides slab_strides(int layout) {
    return layout == DENSE || layout == PACKED || layout == VALUES ? SLAB_STRIDES[layout] : SlabStrides{0, 0, 0, 0, 0, 0, 0};
}
// A kernel parameter block (or CheckGeo) carries six of them under these names.
template <class P>
constexpr void set_strides(P &p, const SlabStrides &st) {
    p.sx = st.x; p.sy = st.y; p.sz = st.z;
    p.kxs = st.kx; p.kys = st.ky; p.kzs = st.kz;
}

// Closed forms of the dense-row -> packed-index maps (the prefix counts of encrypt_assigned_mask / key_assigned_mask
// above; -1 = the row is never assigned in that column).  The assemble kernels use these instead of a table so that a
// cell is a chain of two loads (slab byte -> Fr LUT), not three; the static_assert below and tests/test_lane_model.py
// check them row by row against the masks.
AESW_HD constexpr int packed_index_enc(int c, int r) {
    if (c == 0) return r;
    if (r < 16) return -1;
    if (r < 32) return r - 16;
    if (r >= 1328) {  // round 10: S-box rows (x, y), then the last AddRoundKey (x, y, z)
        if (r < 1344) return c == 1 ? 1024 + (r - 1328) : -1;
        return (c == 1 ? 1040 : 592) + (r - 1344);
    }
    const int R1 = (r - 32) / 144, q = (r - 32) - 144 * R1;  // rounds 1..9: 112 y and 64 z per round
    const int base = 16 + (c == 1 ? 112 : 64) * R1;
    if (q < 16) return c == 1 ? base + q : -1;                       // SubBytes
    if (q >= 128) return base + (c == 1 ? 96 : 48) + (q - 128);      // AddRoundKey
    const int k = (q - 16) / 7, t = (q - 16) - 7 * k;                 // MixColumns record k, row t of 7
    if (t >= 4) return c == 1 ? base + 18 + 5 * k + (t - 4) : base + 3 * k + (t - 4);
    if (c == 2) return -1;
    const int m = k & 3;  // the two products of MIX row m sit at t = m, m + 1 (m = 3: t = 0, 3)
    const int first = m == 3 ? 0 : m, second = m == 3 ? 3 : m + 1;
    return t == first ? base + 16 + 5 * k : t == second ? base + 17 + 5 * k : -1;
}

AESW_HD constexpr int packed_index_key(int c, int r) {
    if (c == 0) return r;
    const int rho = r / 40, j = r - 40 * rho;
    if (c == 1) return j < 24 ? 24 * rho + j : -1;
    return (j >= 4 && j < 24) ? 20 * rho + (j - 4) : -1;
}

constexpr bool closed_forms_are_the_prefix_counts() {
    for (int c = 0; c < 3; ++c) {
        uint8_t em[AES_ROWS] = {}, km[KEY_ROWS] = {};
        int ei[AES_ROWS] = {}, ki[KEY_ROWS] = {};
        encrypt_assigned_mask(c, em);
        key_assigned_mask(c, km);
        mask_to_index(em, AES_ROWS, ei);
        mask_to_index(km, KEY_ROWS, ki);
        for (int r = 0; r < AES_ROWS; ++r)
            if (packed_index_enc(c, r) != ei[r]) return false;
        for (int r = 0; r < KEY_ROWS; ++r)
            if (packed_index_key(c, r) != ki[r]) return false;
    }
    return true;
}
static_assert(closed_forms_are_the_prefix_counts(), "packed_index_enc / packed_index_key left the classifiers' prefix counts");

// ---- equality constraints (the permutation argument), input independent --------------------------------
// Every copy_advice() of one encrypt() call / of schedule_keys(), in the reference's call order.  Cells live in one of
// three spaces: 0 = the block's slab (columns x/y/z of its column set, block-relative row), 1 = the key slab (columns
// x/y/z of set 0, rows 0..399), 2 = words_column (rows 0..95).  The graphs say how cells are related, not which cells
// exist, so they keep a walk of their own; the map only says how many edges there are: every x cell below the sixteen
// plaintext rows and every y cell of an xor row is the destination of exactly one copy_advice(), and so is each of the
// 4 shifted words_column rows of a key round.
struct CopyEdge {
    uint8_t dst_space, dst_col;
    uint16_t dst_row;
    uint8_t src_space, src_col;
    uint16_t src_row;
};
struct CellRef { uint8_t space, col; uint16_t row; };
constexpr int BLOCK_COPIES = 1952;
constexpr int KEY_COPIES = 640;
static_assert(BLOCK_COPIES == (int)(slab_strides(PACKED).x - 16 + slab_strides(PACKED).z), "block copies: x below the plaintext rows + y of the xor rows");
static_assert(KEY_COPIES == (int)(slab_strides(PACKED).kx + slab_strides(PACKED).kz + 4 * (KEY_ROWS / 40)), "key copies: kx + ky of the xor rows + shifted words");

// round-key byte idx of round `round` as schedule_keys() returns it: the key bytes in words_column, later rounds the z
// cells of the word xor rows (src/key_schedule.rs:197-216)
inline CellRef round_key_cell(int round, int idx) {
    if (round == 0) return CellRef{2, 0, (uint16_t)idx};
    return CellRef{1, 2, (uint16_t)(40 * (round - 1) + 8 + idx)};
}

inline int block_copy_graph(CopyEdge *e) {
    int n = 0;
    auto copy = [&](CellRef src, uint8_t col, int row) {
        e[n++] = CopyEdge{0, col, (uint16_t)row, src.space, src.col, src.row};
        return CellRef{0, col, (uint16_t)row};
    };
    CellRef s[16];
    for (int i = 0; i < 16; ++i) {  // src/aes128.rs:194-198
        copy(CellRef{0, 0, (uint16_t)i}, 0, 16 + i);
        copy(round_key_cell(0, i), 1, 16 + i);
        s[i] = CellRef{0, 2, (uint16_t)(16 + i)};
    }
    for (int R = 1; R <= 10; ++R) {
        const int B = R <= 9 ? 32 + 144 * (R - 1) : 1328;
        CellRef sub[16], mixed[16];
        for (int i = 0; i < 16; ++i) {  // :203-209
            copy(s[i], 0, B + i);
            sub[i] = CellRef{0, 1, (uint16_t)(B + i)};
        }
        if (R <= 9) {
            for (int w = 0; w < 4; ++w)
                for (int m = 0; m < 4; ++m) {  // lcon(), :268-301
                    const int base = B + 16 + 7 * (4 * w + m);
                    CellRef tmp[4];
                    for (int t = 0; t < 4; ++t) {
                        const CellRef c = copy(sub[4 * ((w + t) % 4) + t], 0, base + t);
                        tmp[t] = MIX[m][t] == 1 ? c : CellRef{0, 1, (uint16_t)(base + t)};
                    }
                    copy(tmp[0], 0, base + 4); copy(tmp[1], 1, base + 4);
                    copy(tmp[2], 0, base + 5); copy(tmp[3], 1, base + 5);
                    copy(CellRef{0, 2, (uint16_t)(base + 4)}, 0, base + 6);
                    copy(CellRef{0, 2, (uint16_t)(base + 5)}, 1, base + 6);
                    mixed[4 * w + m] = CellRef{0, 2, (uint16_t)(base + 6)};
                }
        } else {
            for (int w = 0; w < 4; ++w)
                for (int j = 0; j < 4; ++j) mixed[4 * w + j] = sub[4 * ((w + j) % 4) + j];  // :236-237
        }
        const int A = R <= 9 ? B + 128 : 1344;
        for (int i = 0; i < 16; ++i) {  // :250-261
            copy(mixed[i], 0, A + i);
            copy(round_key_cell(R, i), 1, A + i);
            s[i] = CellRef{0, 2, (uint16_t)(A + i)};
        }
    }
    return n;
}

inline int key_copy_graph(CopyEdge *e) {
    int n = 0;
    auto copy = [&](CellRef src, uint8_t space, uint8_t col, int row) {
        e[n++] = CopyEdge{space, col, (uint16_t)row, src.space, src.col, src.row};
        return CellRef{space, col, (uint16_t)row};
    };
    for (int rho = 1; rho <= 10; ++rho) {  // assign_round, src/key_schedule.rs:122-224
        const int B = 40 * (rho - 1), W = 16 + 8 * (rho - 1);
        static const int rot[4] = {13, 14, 15, 12};
        CellRef shifted[4], rconned[4], next[4];
        for (int i = 0; i < 4; ++i) shifted[i] = copy(round_key_cell(rho - 1, rot[i]), 2, 0, W + i);   // :141-154
        for (int i = 0; i < 4; ++i) copy(shifted[i], 1, 0, B + i);                                      // sbox rows
        for (int i = 0; i < 4; ++i) {                                                                   // :189-194
            copy(CellRef{1, 1, (uint16_t)(B + i)}, 1, 0, B + 4 + i);
            copy(CellRef{2, 0, (uint16_t)(W + 4 + i)}, 1, 1, B + 4 + i);
            rconned[i] = CellRef{1, 2, (uint16_t)(B + 4 + i)};
        }
        for (int i = 0; i < 4; ++i) {                                                                   // :197-204
            copy(round_key_cell(rho - 1, i), 1, 0, B + 8 + i);
            copy(rconned[i], 1, 1, B + 8 + i);
            next[i] = CellRef{1, 2, (uint16_t)(B + 8 + i)};
        }
        for (int wd = 1; wd < 4; ++wd)                                                                  // :207-216
            for (int i = 0; i < 4; ++i) {
                copy(round_key_cell(rho - 1, 4 * wd + i), 1, 0, B + 8 + 4 * wd + i);
                copy(next[i], 1, 1, B + 8 + 4 * wd + i);
                next[i] = CellRef{1, 2, (uint16_t)(B + 8 + 4 * wd + i)};
            }
        for (int i = 0; i < 16; ++i) copy(CellRef{1, 2, (uint16_t)(B + 8 + i)}, 1, 0, B + 24 + i);      // :218-221
    }
    return n;
}

}  // namespace aesw
