// aesw_check_dev.h -- the wave-level core of the device witness checker, one source for all three checker kernels: check_kernel
// (aesw_kernels.hip, libaesw.so), circ_check_kernel (circ/aesw_circ_check.hip, libaesw_circ.so) and cols_check_kernel
// (cols/aesw_cols_check.hip, libaesw_cols.so).  aesw_check.h holds the checks themselves (the exact walk the CPU model runs);
// this header holds what decides on the device whether a staged unit passes: the wave's LDS synchronisation, the register
// staging of a unit's column ranges, the fast path's form of the check table and its branch-free walk, the verdict of a staged
// block and of a staged key unit (block_unit_check, key_unit_check), the validation of circuit offsets (offsets_bad) and the
// flush of a lane's counts into the report (flush_acc; the report's reset is aesw_report_dev.h's).  A kernel adds its prologue and its staging loop: how a unit and its
// literal bytes get into the image and into registers.  The launch geometry the three launchers share is host code and lives
// in aesw_internal.h.  Device code only: include from a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "aesw_internal.h"
#include "aesw_check.h"
#include "aesw_report_dev.h"  // LANES, report_reset
#include "aesw_store.h"       // u32x4, u32x2

namespace aesw {

// a value every lane of the wave holds alike, said so to the compiler: what is derived from it stays in scalar registers
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32 | __builtin_amdgcn_readfirstlane((uint32_t)v);
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One column range of a unit on its way from global memory into the wave's LDS image: BYTES bytes as units of VEC bytes (16 where the
// layout's strides keep both sides 16-byte aligned, 8 for the packed kz and words_column), unit lane + 64 j in lane's j-th register.
// load() only issues the loads; store() is called a block later, so the next unit's bytes travel while the current one is checked.
template <int BYTES, int VEC>
struct Staged {
    static_assert(BYTES % VEC == 0 && (VEC == 16 || VEC == 8), "whole units");
    static constexpr int UNITS = BYTES / VEC, N = (UNITS + LANES - 1) / LANES;
    using V = typename std::conditional<VEC == 16, u32x4, u32x2>::type;
    V v[N];
    __device__ __forceinline__ void load(const uint8_t *src, uint32_t lane) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t i = lane + LANES * j;
            if (i < (uint32_t)UNITS) v[j] = reinterpret_cast<const V *>(src)[i];
        }
    }
    __device__ __forceinline__ void store(uint8_t *dst, uint32_t lane) const {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t i = lane + LANES * j;
            if (i < (uint32_t)UNITS) reinterpret_cast<V *>(dst)[i] = v[j];
        }
    }
};

// The fast path's form of the check table, in LDS (one copy per workgroup): offsets of cells a layout leaves out (CHECK_NONE; only
// on rows whose tag does not read them) point at byte 0, tags that cannot fail (no lookup, U8 range) become 0, and a row entry
// carries the offset of its value table inside t768:  w0 = ox | oy << 16,  w1 = oz | tag << 16 | table offset << 20.
__device__ __forceinline__ void fast_row_entry(uint32_t a, uint32_t b, uint32_t &w0, uint32_t &w1) {
    const uint32_t tag = b >> 16;
    const uint32_t ox = (a & 0xffffu) == CHECK_NONE ? 0u : (a & 0xffffu), oy = (a >> 16) == CHECK_NONE ? 0u : (a >> 16),
                   oz = (b & 0xffffu) == CHECK_NONE ? 0u : (b & 0xffffu);
    const uint32_t tg = tag < 2 ? 0u : tag;
    w0 = ox | oy << 16;
    w1 = oz | tg << 16 | (tg >= 3 ? (tg - 3) * 256u : 0u) << 20;
}
__device__ __forceinline__ void load_fast_table(uint32_t *tab, const uint32_t *t) {
    for (uint32_t r = threadIdx.x; r < (uint32_t)(AES_ROWS + KEY_ROWS); r += blockDim.x) {
        const uint32_t base = r < (uint32_t)AES_ROWS ? CHK_ROWS + 2 * r : CHK_KROWS + 2 * (r - AES_ROWS);
        fast_row_entry(t[base], t[base + 1], tab[base], tab[base + 1]);
    }
    for (uint32_t i = threadIdx.x; i < (uint32_t)BLOCK_COPIES; i += blockDim.x) tab[CHK_EDGES + i] = t[CHK_EDGES + i];
    for (uint32_t i = threadIdx.x; i < (uint32_t)(KEY_COPIES + WORDS_ROWS); i += blockDim.x) tab[CHK_KEDGES + i] = t[CHK_KEDGES + i];
}
// Table words whose low half is the image offset of a literal row a lane compares in the fast path (lanes 0..15, i = lane & 15;
// the other lanes read a valid entry they never use).  Ciphertext: z of the block's last sixteen rows, AES_ROWS - 16 + i, which
// sits in the second word of the row entry: tab[CHK_CT_LITERALS + 2 * i].  Key bytes: words_column rows 0..15, the low half of
// their gate entries: tab[CHK_KEY_LITERALS + i].  Constants, not helpers: a function around the index or the load compiles
// check_kernel differently (profiles/checker_core/README.md).
constexpr int CHK_CT_LITERALS = CHK_ROWS + 2 * (AES_ROWS - 16) + 1, CHK_KEY_LITERALS = CHK_GATES;

// one lookup row, branch-free: 1 if the enabled lookup has no table row
__device__ __forceinline__ uint32_t fast_row_bad(const uint8_t *img, const uint8_t *t768, uint32_t w0, uint32_t w1) {
    const uint32_t x = img[w0 & 0xffffu], y = img[w0 >> 16], z = img[w1 & 0xffffu], tag = (w1 >> 16) & 7u;
    const uint32_t lk = t768[(w1 >> 20) + x];
    const uint32_t want = tag == 2 ? (x ^ y) : lk, got = tag == 2 ? z : y;
    return (tag != 0) & (want != got);
}
template <int ROWS_AT, int NROWS, int EDGES_AT, int NEDGES>
__device__ __forceinline__ uint32_t fast_unit_bad(const uint8_t *img, const uint8_t *t768, const uint32_t *tab, uint32_t lane) {
    uint32_t bad = 0;
    const uint2 *rows = reinterpret_cast<const uint2 *>(tab + ROWS_AT);
#pragma unroll 4
    for (uint32_t r = lane; r < (uint32_t)NROWS; r += LANES) {
        const uint2 w = rows[r];
        bad |= fast_row_bad(img, t768, w.x, w.y);
    }
#pragma unroll 4
    for (uint32_t e = lane; e < (uint32_t)NEDGES; e += LANES) {
        const uint32_t d = tab[EDGES_AT + e];
        bad |= img[d & 0xffffu] != img[d >> 16];
    }
    return bad;
}

// Fast path per unit: every lane evaluates its slice branch-free out of registers ("is anything wrong with this unit?"); only a
// unit where some lane says yes is walked again by the exact code of aesw_check.h (the code the CPU model runs), which counts
// and names the failures.  A satisfied witness -- the normal case -- never takes the second walk.
// Pipeline per wave: the loads of block b + stride are issued (into registers) before block b is checked out of LDS.
// img: the wave's image with the unit staged and wave_lds_sync() passed; tab / t768: the fast table and tab768 in LDS;
// table: the check table in global memory, which the exact walk reads; lit_b: plaintext | ciphertext << 8 and klit: the key byte
// of lanes 0..15, fetched with the unit; ct_off / w_off: the offsets out of tab[CHK_CT_LITERALS + 2 * i] / tab[CHK_KEY_LITERALS + i].
__device__ __forceinline__ void block_unit_check(const uint8_t *img, const uint32_t *tab, const uint8_t *t768, const uint32_t *table,
                                                 const uint8_t *pt, const uint8_t *ct, uint32_t lit_b, uint32_t ct_off, uint64_t b,
                                                 uint32_t lane, CheckAcc &acc) {
    uint32_t bad = fast_unit_bad<CHK_ROWS, AES_ROWS, CHK_EDGES, BLOCK_COPIES>(img, t768, tab, lane);
    if (lane < 16) {
        bad |= img[lane] != (lit_b & 0xffu);
        if (ct) bad |= img[ct_off] != (lit_b >> 8);
    }
    if (__ballot(bad != 0) != 0) check_block(img, table, t768, pt + b * 16, ct ? ct + b * 16 : nullptr, b, lane, LANES, acc);
}
__device__ __forceinline__ void key_unit_check(const uint8_t *img, const uint32_t *tab, const uint8_t *t768, const uint32_t *table,
                                               const uint8_t *keys, uint32_t klit, uint32_t w_off, uint64_t unit, uint32_t lane,
                                               CheckAcc &acc) {
    uint32_t kbad = fast_unit_bad<CHK_KROWS, KEY_ROWS, CHK_KEDGES, KEY_COPIES>(img, t768, tab, lane);
    for (uint32_t r = lane; r < (uint32_t)WORDS_ROWS; r += LANES) {
        const uint32_t gte = tab[CHK_GATES + r];
        kbad |= ((gte >> 24) != 0) & (img[gte & 0xffffu] != ((gte >> 16) & 0xffu));
    }
    if (lane < 16 && keys) kbad |= img[w_off] != klit;
    if (__ballot(kbad != 0) != 0) check_key(img, table, t768, keys ? keys + unit * 16 : nullptr, unit, lane, LANES, acc);
}
// One lane's finding into a word of the report.  Failures are the rare case: a lane that found any adds them itself.
__device__ __forceinline__ void report_add(uint64_t *word, uint64_t count) {
    if (count) atomicAdd(reinterpret_cast<unsigned long long *>(word), (unsigned long long)count);
}
__device__ __forceinline__ void report_min(uint64_t *word, uint64_t first) {
    if (first != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(word), (unsigned long long)first);
}
// report words 2..6 (lookup, copy, gate, input, first); a kernel whose report has more words adds them next to the call
__device__ __forceinline__ void flush_acc(uint64_t *report, const CheckAcc &acc) {
    report_add(report + 2, acc.lookup); report_add(report + 3, acc.copy); report_add(report + 4, acc.gate); report_add(report + 5, acc.input);
    report_min(report + 6, acc.first);
}
// The circuit offsets of a many-circuit batch (C + 1 values: 0 first, n last, ascending, at most `cap` blocks per circuit),
// validated by the lanes of the grid, one circuit per lane, once: what this lane counted.
__device__ __forceinline__ uint32_t offsets_bad(const uint64_t *offsets, uint64_t nc, uint64_t n, uint64_t cap, uint64_t gwave,
                                                uint64_t nwaves, uint32_t lane) {
    uint32_t off_bad = 0;
    for (uint64_t c = gwave * LANES + lane; c < nc; c += nwaves * LANES) {
        const uint64_t o0 = offsets[c], o1 = offsets[c + 1];
        off_bad += (o1 < o0 || o1 - o0 > cap) ? 1u : 0u;
        if (c == 0 && o0 != 0) ++off_bad;
        if (c + 1 == nc && o1 != n) ++off_bad;
    }
    return off_bad;
}

template <int LAYOUT>
struct ChkLayout {
    static constexpr SlabStrides ST = slab_strides(LAYOUT == DENSE ? DENSE : PACKED);  // check_geo's domain
    static constexpr int SX = ST.x, SY = ST.y, SZ = ST.z, KXS = ST.kx, KYS = ST.ky, KZS = ST.kz;
    static constexpr int BI = ST.block_bytes(), O_KY = KXS, O_KZ = KXS + KYS, O_W = KXS + KYS + KZS, KI = ST.key_bytes();
    static constexpr int IMG = (BI + KI + 15) / 16 * 16;
    static constexpr int KZV = KZS % 16 == 0 && (BI + O_KZ) % 16 == 0 ? 16 : 8, WV = (BI + O_W) % 16 == 0 ? 16 : 8;
    static_assert(SX % 16 == 0 && SY % 16 == 0 && SZ % 16 == 0 && KXS % 16 == 0 && KYS % 16 == 0 && BI % 16 == 0, "16-byte units");
};

template <int LAYOUT>
struct StagedKey {
    using G = ChkLayout<LAYOUT>;
    Staged<G::KXS, 16> kx; Staged<G::KYS, 16> ky; Staged<G::KZS, G::KZV> kz; Staged<WORDS_ROWS, G::WV> w;
    __device__ __forceinline__ void load(const CheckParams &a, uint64_t k, uint32_t lane) {
        kx.load(a.kx + k * G::KXS, lane); ky.load(a.ky + k * G::KYS, lane); kz.load(a.kz + k * G::KZS, lane); w.load(a.kw + k * WORDS_ROWS, lane);
    }
    __device__ __forceinline__ void store(uint8_t *kimg, uint32_t lane) const {
        kx.store(kimg, lane); ky.store(kimg + G::O_KY, lane); kz.store(kimg + G::O_KZ, lane); w.store(kimg + G::O_W, lane);
    }
};

}  // namespace aesw
