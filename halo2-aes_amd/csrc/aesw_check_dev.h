// aesw_check_dev.h -- the device building blocks of the witness checker (aesw_check.h holds the checks themselves): the wave's
// LDS synchronisation, the register staging of a unit's column ranges, the fast path's form of the check table and its
// branch-free walk.  One source for every checker kernel: check_kernel (aesw_kernels.hip, libaesw.so) and circ_check_kernel
// (circ/aesw_circ_check.hip, libaesw_circ.so).  Device code only: include from a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "aesw_internal.h"
#include "aesw_check.h"

namespace aesw {

constexpr int LANES = 64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

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

// Fast path per block: every lane evaluates its slice branch-free out of registers ("is anything wrong with this unit?"); only a
// unit where some lane says yes is walked again by the exact code of aesw_check.h (the code the CPU model runs), which counts
// and names the failures.  A satisfied witness -- the normal case -- never takes the second walk.
// Pipeline per wave: the loads of block b + stride are issued (into registers) before block b is checked out of LDS.
template <int LAYOUT>
struct ChkLayout {
    static constexpr int SX = AES_ROWS, SY = LAYOUT == DENSE ? AES_ROWS : Geo<PACKED>::YS, SZ = LAYOUT == DENSE ? AES_ROWS : Geo<PACKED>::ZS;
    static constexpr int KXS = KEY_ROWS, KYS = LAYOUT == DENSE ? KEY_ROWS : Geo<PACKED>::KYS, KZS = LAYOUT == DENSE ? KEY_ROWS : Geo<PACKED>::KZS;
    static constexpr int BI = SX + SY + SZ, O_KY = KXS, O_KZ = KXS + KYS, O_W = KXS + KYS + KZS, KI = O_W + WORDS_ROWS;
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
