// aesw_layout.h -- geometry of the witness slabs as the kernels write them: where the pieces of a column sit inside a
// block (Geo) and inside its LDS staging window (Win).  Shared by the HIP kernels and the host-side lane model used by
// the tests.  Which rows and cells exist at all is aesw_slabmap.h's; the byte counts here are pinned to it below.
#pragma once
#include "aesw_slabmap.h"

namespace aesw {

// ---- encrypt slab -----------------------------------------------------------
// Per column: HEAD bytes (rows 0..31: plaintext rows + initial AddRoundKey,
// src/aes128.rs:176-198), nine ROUND-sized pieces (rounds 1..9, :201-262) and
// TAIL bytes (round 10).  Inside a round: SBOX rows, 16 lcon() records of
// MIXW/4... bytes per lane-word, ARK rows.
template <int L>
struct Geo {
    static constexpr bool HAS_X = L != VALUES;      // column x is emitted at all
    static constexpr bool Y_COPIES = L != VALUES;   // y cells of xor rows (round keys, tmp1/tmp3/i2) are emitted
    // bytes per block
    static constexpr int XS = HAS_X ? 1360 : 0;
    static constexpr int YS = L == DENSE ? 1360 : L == PACKED ? 1056 : 448;
    static constexpr int ZS = L == DENSE ? 1360 : 608;
    // head / round / tail bytes
    static constexpr int X_HEAD = 32, X_ROUND = 144, X_TAIL = 32;
    static constexpr int Y_HEAD = L == DENSE ? 32 : L == PACKED ? 16 : 0, Y_ROUND = L == DENSE ? 144 : L == PACKED ? 112 : 48,
                         Y_TAIL = L == VALUES ? 16 : 32;
    static constexpr int Z_HEAD = L == DENSE ? 32 : 16, Z_ROUND = L == DENSE ? 144 : 64,
                         Z_TAIL = L == DENSE ? 32 : 16;
    // offsets inside the head (relative to the head start)
    static constexpr int X_H_PT = 0, X_H_ARK = 16;        // rows 0..15 pt, rows 16..31 pt again
    static constexpr int Y_H_ARK = L == DENSE ? 16 : 0;   // rk0
    static constexpr int Z_H_ARK = L == DENSE ? 16 : 0;   // pt ^ rk0
    // offsets inside a round (relative to the round start)
    static constexpr int X_SBOX = 0, X_MIX = 16, X_MIXW = 28, X_ARK = 128;
    static constexpr int Y_SBOX = 0, Y_MIX = 16, Y_MIXW = L == DENSE ? 28 : L == PACKED ? 20 : 8,
                         Y_ARK = L == DENSE ? 128 : 96 /* not in VALUES */;
    static constexpr int Z_SBOX = 0 /* dense only: zeros */, Z_MIX = L == DENSE ? 16 : 0,
                         Z_MIXW = L == DENSE ? 28 : 12, Z_ARK = L == DENSE ? 128 : 48;
    // offsets inside the tail (round 10: sbox rows, then ShiftRows ^ rk10)
    static constexpr int X_T_SBOX = 0, X_T_ARK = 16;
    static constexpr int Y_T_SBOX = 0, Y_T_ARK = 16 /* not in VALUES */;
    static constexpr int Z_T_ARK = L == DENSE ? 16 : 0;
    // dwords per lcon record group of one lane-word (4 output bytes x 7 rows)
    static constexpr int X_MIXD = 7, Y_MIXD = L == DENSE ? 7 : L == PACKED ? 5 : 2, Z_MIXD = L == DENSE ? 7 : 3;

    // ---- key slab (per key): rounds of KX_ROUND bytes, no head.  VALUES keeps the PACKED key slab (one key
    // slab per circuit in the reference's call shape; nothing to save there)
    static constexpr int KXS = 400;
    static constexpr int KYS = L == DENSE ? 400 : 240;
    static constexpr int KZS = L == DENSE ? 400 : 200;
    static constexpr int KX_ROUND = 40, KY_ROUND = L == DENSE ? 40 : 24, KZ_ROUND = L == DENSE ? 40 : 20;
    // kz packed drops rows 0..3 of every round (sbox rows have no z)
    static constexpr int KZ_SHIFT = L == DENSE ? 0 : 4;
};
// the bytes per block / per key the emit code works with are the cells the slab map counts
template <int L>
constexpr bool geo_is_the_slab_map() {
    using G = Geo<L>;
    constexpr SlabStrides st = slab_strides(L);
    return G::XS == (int)st.x && G::YS == (int)st.y && G::ZS == (int)st.z && G::KXS == (int)st.kx && G::KYS == (int)st.ky && G::KZS == (int)st.kz;
}
static_assert(geo_is_the_slab_map<DENSE>() && geo_is_the_slab_map<PACKED>() && geo_is_the_slab_map<VALUES>(), "Geo<L>::XS ... KZS left the slab map's counts");

// LDS staging window of one block, one column (DESIGN.md "staging window").
// HBM wants whole 128-byte lines: per-round runs (144/112/64 B at 16-byte
// alignment) write every line two or three times partially and cap at ~3 TB/s,
// whole lines reach ~5.5 TB/s (tools/storebench.hip).  So after every round a
// wave flushes only the lines that are complete; the <=112 not yet flushed
// bytes of a block stay in LDS.  Window layout (bytes, block-relative offset o):
//   [0, PERM_END)            head + the first PERM_R rounds, kept until the end:
//                            the first (<128) bytes of a block share a line with
//                            the previous block's tail, which completes last
//   NSLOT slots of ROUND     rounds PERM_R+1..9, slot = (R-PERM_R-1) % NSLOT
//   TAIL                     round 10
// padded to BYTES = 16 (mod 32) so that the same offset of the 8 blocks of a
// half-wave falls on 8 different 4-bank groups (conflict-free ds_write_b32).
template <int HEAD_, int ROUND_, int TAIL_, int GSTRIDE_>
struct Win {
    static constexpr int HEAD = HEAD_, ROUND = ROUND_, TAIL = TAIL_, GSTRIDE = GSTRIDE_;
    static constexpr int PERM_R = HEAD + ROUND >= 128 ? 1 : (HEAD + 2 * ROUND >= 128 ? 2 : 3);
    static constexpr int NSLOT = 1 + (112 + ROUND - 1) / ROUND;  // rounds that can hold unflushed bytes, +1 being written
    static constexpr int PERM_END = HEAD + PERM_R * ROUND;
    static constexpr int SLOT0 = PERM_END;
    static constexpr int TAIL0 = SLOT0 + NSLOT * ROUND;
    static constexpr int RAW = TAIL0 + TAIL;
    static constexpr int BYTES = RAW + ((16 - RAW % 32) + 32) % 32;
    static_assert(HEAD + 9 * ROUND + TAIL == GSTRIDE, "column geometry");
    static_assert(HEAD % 16 == 0 && ROUND % 16 == 0 && TAIL % 16 == 0 && GSTRIDE % 16 == 0, "16-byte pieces");
    static_assert((16 * GSTRIDE) % 128 == 0, "a wave's 16-block range is line aligned");
    // block-relative offset where round R starts (R = 10: the tail) / ends
    AESW_HD static constexpr int start(int R) { return HEAD + ROUND * (R - 1); }
    AESW_HD static constexpr int end(int R) { return R >= 10 ? GSTRIDE : HEAD + ROUND * R; }
    // window offset where round R's bytes are staged
    AESW_HD static constexpr int woff(int R) {
        return R <= PERM_R ? start(R) : (R >= 10 ? TAIL0 : SLOT0 + ((R - PERM_R - 1) % NSLOT) * ROUND);
    }
};
template <int L> using WinX = Win<Geo<L>::X_HEAD, Geo<L>::X_ROUND, Geo<L>::X_TAIL, 1360>;  // VALUES: a valid type, never staged
template <int L> using WinY = Win<Geo<L>::Y_HEAD, Geo<L>::Y_ROUND, Geo<L>::Y_TAIL, Geo<L>::YS>;
template <int L> using WinZ = Win<Geo<L>::Z_HEAD, Geo<L>::Z_ROUND, Geo<L>::Z_TAIL, Geo<L>::ZS>;


// Which kernel writes the Fr form of aesw_assemble_advice_* for a K / column count under option "assemble_geometry": 0 = the
// striding kernel (any shape), 1 = one-shot workgroups on a (chunk, segment, column) grid -- needs 1 + ceil(2^K / 1360) <= 65535
// segments in grid.y --, 2 = one-shot workgroups on aligned chunks (geometries 2 / 3 / 4: 8 <= K <= 30).  A geometry that cannot
// cover the shape falls back to the striding kernel: an option never turns a valid call into an error.
inline int assemble_kernel_choice(bool as_fr, int geometry, uint32_t k, uint32_t col_count) {
    if (!as_fr || col_count == 0) return 0;
    if (geometry == 1) {
        const uint64_t rows = (uint64_t)1 << k;
        const uint64_t segs = 1 + (rows + AES_ROWS - 1) / AES_ROWS;
        return segs <= 65535 && col_count <= 65535 ? 1 : 0;
    }
    if (geometry >= 2) return k >= 8 && k <= 30 && col_count <= 65535 ? 2 : 0;
    return 0;
}

}  // namespace aesw
