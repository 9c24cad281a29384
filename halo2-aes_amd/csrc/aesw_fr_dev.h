// aesw_fr_dev.h -- what the kernels of every library that computes in Fr do to a cell alike, once: a cell between
// memory and registers (load_cell, store_cell, cell_at), a cell between the lanes of a wave (shfl_*_cell) and the inclusive scans
// of a wave (wave_scan_up, wave_scan_down).  The field is aesw_fr.h's.  Bodies only, no LDS and no barrier: how the waves of a
// workgroup meet stays in the kernels (4.24 says why).  Device code only, and no __global__, for the reason aesw_report_dev.h gives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aesw_fr.h"
#include "aesw_report_dev.h"
#include "aesw_store.h"

namespace aesw {

// ---- a cell and memory: two 16-byte pieces, cell i of a column 32 i bytes behind its base ----------------------------------------

__device__ __forceinline__ Fr load_cell(const u32x4 *p) {
    const u32x4 lo = p[0], hi = p[1];
    return Fr{{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
}
template <int NT>  // aesw_store.h's flavour
__device__ __forceinline__ void store_cell(u32x4 *p, const Fr &v) {
    gstore<NT>(p, u32x4{v.l[0], v.l[1], v.l[2], v.l[3]});
    gstore<NT>(p + 1, u32x4{v.l[4], v.l[5], v.l[6], v.l[7]});
}
__device__ __forceinline__ const u32x4 *cell_at(const u32x4 *base, uint64_t i) { return base + i * 2; }
__device__ __forceinline__ u32x4 *cell_at(u32x4 *base, uint64_t i) { return base + i * 2; }

// ---- a cell and the wave ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ Fr shfl_up_cell(const Fr &v, int o) {
    Fr r = FR_ZERO;
#pragma unroll
    for (int i = 0; i < FR_LIMBS; ++i) r.l[i] = __shfl_up(v.l[i], o, LANES);
    return r;
}
__device__ __forceinline__ Fr shfl_down_cell(const Fr &v, int o) {
    Fr r = FR_ZERO;
#pragma unroll
    for (int i = 0; i < FR_LIMBS; ++i) r.l[i] = __shfl_down(v.l[i], o, LANES);
    return r;
}
__device__ __forceinline__ Fr shfl_xor_cell(const Fr &v, int o) {
    Fr r = FR_ZERO;
#pragma unroll
    for (int i = 0; i < FR_LIMBS; ++i) r.l[i] = __shfl_xor(v.l[i], o, LANES);
    return r;
}

// The inclusive scan of one cell per lane over a wave: upwards lane l ends with the product of lanes 0 ... l, downwards with that
// of lanes l ... 63.  Every lane shuffles; the lanes that have a partner multiply.
__device__ __forceinline__ Fr wave_scan_up(Fr v, uint32_t lane) {
#pragma unroll 1
    for (int o = 1; o < LANES; o <<= 1) {
        const Fr other = shfl_up_cell(v, o);
        if (lane >= (uint32_t)o) v = fr_mul(other, v);
    }
    return v;
}
__device__ __forceinline__ Fr wave_scan_down(Fr v, uint32_t lane) {
#pragma unroll 1
    for (int o = 1; o < LANES; o <<= 1) {
        const Fr other = shfl_down_cell(v, o);
        if (lane + (uint32_t)o < (uint32_t)LANES) v = fr_mul(other, v);
    }
    return v;
}

}  // namespace aesw
