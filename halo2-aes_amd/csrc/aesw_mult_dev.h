// aesw_mult_dev.h -- the wave-level core of counting lookup multiplicities, one source for the kernels of libaesw_mult.so
// (mult/aesw_mult.hip), libaesw_acc.so (acc/aesw_acc.hip) and libaesw_vacc.so (vacc/aesw_vacc.hip).  aesw_mult.h holds the rule
// (bins, hits, the sizes of the counter split); aesw_check_dev.h how a slab travels (Staged) and how a wave synchronises on its
// LDS image.  This header holds what counts a staged unit: a lane's findings, a row of the check table as the walk reads it, the
// two sinks a hit goes to (a global atomic add; the workgroup's LDS counters, and with them which workgroup of a pair owns
// which bin), the staging of a block and the 22 rows a lane keeps of it, the key slab of one wave, the workgroup's report and
// the wave count that fits next to the counters; the add flush of both accumulators (flush_add, flush_pair_add); and the body
// that zeroes histograms and resets a report (zero_and_reset: a library's kernel of its own name wraps it; a __global__ here
// would be a kernel of every library that includes this).  A kernel adds its prologue and its staging loop -- which blocks,
// which unit numbers: that loop stays in the kernels ("Shared machinery").  Device code only (what the entry
// points share is aesw_entry.h's): include from a HIP translation unit.
#pragma once
#include "../../include/aesw_mult.h"
#include "aesw_check_dev.h"
#include "aesw_mult.h"

namespace aesw {
namespace multdev {

// What one lane found: enabled lookups, misses and the smallest miss (CheckAcc's key, kind CHK_LOOKUP).
struct Findings {
    uint32_t lookups = 0, misses = 0;  // a lane sees at most 22 rows of 2^30 / AES_ROWS blocks
    uint64_t first = ~0ull;
};

// A row entry of the check table with its offsets taken relative to `base` (0: a block image, BI: a key image on its own);
// a cell the layout leaves out (CHECK_NONE: the rule never reads it on that row) points at byte 0.
__device__ __forceinline__ void row_entry(const uint32_t *t, uint32_t at, uint32_t base, uint32_t &w0, uint32_t &w1) {
    const uint32_t a = t[at], b = t[at + 1];
    const uint32_t ox = (a & 0xffffu) == CHECK_NONE ? 0u : (a & 0xffffu) - base, oy = (a >> 16) == CHECK_NONE ? 0u : (a >> 16) - base,
                   oz = (b & 0xffffu) == CHECK_NONE ? 0u : (b & 0xffffu) - base;
    w0 = ox | oy << 16;
    w1 = oz | (b >> 16) << 16;
}

// One row of a staged unit: the rule of aesw_mult.h, the hit into the sink, the miss into the lane's findings.
template <class Sink>
__device__ __forceinline__ void count_row(const uint8_t *img, const uint8_t *t768, uint32_t w0, uint32_t w1, uint64_t unit, uint32_t is_key,
                                          uint32_t row, Sink &sink, Findings &acc) {
    const uint32_t tag = w1 >> 16;
    const uint32_t x = img[w0 & 0xffffu], y = img[w0 >> 16], z = img[w1 & 0xffffu];
    const bool enabled = tag != 0, hit = mult_hit(tag, x, y, z, t768), miss = enabled && !hit;
    acc.lookups += enabled;
    acc.misses += miss;
    const uint64_t key = unit << 20 | (uint64_t)(is_key << 19 | (uint32_t)CHK_LOOKUP << 16 | row);
    acc.first = miss && key < acc.first ? key : acc.first;
    sink.add(hit, tag, x, y);
}

// one global atomic add per hit (no return value: nothing waits for it)
struct GlobalSink {
    uint32_t *hist;  // of the unit's set
    __device__ __forceinline__ void add(bool hit, uint32_t tag, uint32_t x, uint32_t y) {
        if (hit) atomicAdd(hist + mult_bin(tag, x, y), 1u);
    }
};
// the counters of a workgroup, `half` of its pair: mult_half_owns and mult_counter of aesw_mult.h, whose expressions are kept
// in place here (called as functions they compile to other code); the flushes read mult_flush_range, which
// tests/test_mult_rule.py holds against that rule bin for bin.
struct LdsSink {
    uint32_t *cnt;  // MULT_COUNTERS of them
    uint32_t half;
    __device__ __forceinline__ void add(bool hit, uint32_t tag, uint32_t x, uint32_t y) {  // one predicated ds_add, no branch on the tag
        const uint32_t bin = mult_bin(tag, x, y);
        const bool is_xor = tag == 2;
        const uint32_t at = is_xor ? bin - XOR_FIRST - half * XOR_HALF : XOR_HALF + (bin < XOR_FIRST ? bin : bin - 2 * XOR_HALF);
        if (hit && (is_xor ? (x >> 7) == half : half == 0)) atomicAdd(cnt + at, 1u);
    }
};

// Slabs: a kernel's parameter struct, of which the column pointers x, y, z are read (slab b of a column lies b strides in).
// A template and not a struct of three pointers: the copy is made ahead of the loop, and the counting kernels compile to other
// code.
template <int LAYOUT>
struct BlockStage {
    using G = ChkLayout<LAYOUT>;
    Staged<G::SX, 16> sx; Staged<G::SY, 16> sy; Staged<G::SZ, 16> sz;
    template <class Slabs>
    __device__ __forceinline__ void load(const Slabs &a, uint64_t b, uint32_t lane) {
        sx.load(a.x + b * G::SX, lane); sy.load(a.y + b * G::SY, lane); sz.load(a.z + b * G::SZ, lane);
    }
    __device__ __forceinline__ void store(uint8_t *img, uint32_t lane) const {
        sx.store(img, lane); sy.store(img + G::SX, lane); sz.store(img + G::SX + G::SY, lane);
    }
};
constexpr int ROW_STEPS = (AES_ROWS + LANES - 1) / LANES;  // 22 rows per lane
// The lane's rows of a block, lane + 64 j: their entries, read once.  Past the last row: tag 0, no lookup.
struct BlockRows {
    uint32_t w0[ROW_STEPS], w1[ROW_STEPS];
    __device__ __forceinline__ void load(const uint32_t *table, uint32_t lane) {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) {
            const uint32_t r = lane + LANES * j;
            w0[j] = w1[j] = 0;
            if (r < (uint32_t)AES_ROWS) row_entry(table, CHK_ROWS + 2 * r, 0, w0[j], w1[j]);
        }
    }
    template <class Sink>
    __device__ __forceinline__ void count(const uint8_t *img, const uint8_t *t768, uint64_t b, uint32_t lane, Sink &sink, Findings &acc) const {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) count_row(img, t768, w0[j], w1[j], b, 0, lane + LANES * j, sink, acc);
    }
};

// Key slab c of the key columns by one wave, as unit c: kx | ky | kz into the wave's image (it is smaller than a block's), its
// 400 rows into the sink.  The image is still being read when this returns: a caller that overwrites it synchronises first.
// KeyCols: a kernel's parameter struct with the columns kx, ky, kz and the check table, read where they lie.
template <int LAYOUT, class KeyCols, class Sink>
__device__ __forceinline__ void count_key_slab(const KeyCols &a, uint32_t c, uint8_t *img, const uint8_t *t768, uint32_t lane, Sink &sink, Findings &acc) {
    using G = ChkLayout<LAYOUT>;
    static_assert(G::O_W <= G::BI, "the key columns fit a block image");
    constexpr int KZV = G::KZS % 16 == 0 ? 16 : 8;  // a packed key slab's kz is 200 bytes: slab c starts on an 8-byte boundary
    Staged<G::KXS, 16> kx; Staged<G::KYS, 16> ky; Staged<G::KZS, KZV> kz;
    kx.load(a.kx + (uint64_t)c * G::KXS, lane); ky.load(a.ky + (uint64_t)c * G::KYS, lane); kz.load(a.kz + (uint64_t)c * G::KZS, lane);
    kx.store(img, lane); ky.store(img + G::O_KY, lane); kz.store(img + G::O_KZ, lane);
    wave_lds_sync();
    for (uint32_t r = lane; r < (uint32_t)KEY_ROWS; r += LANES) {
        uint32_t w0, w1;
        row_entry(a.table, CHK_KROWS + 2 * r, G::BI, w0, w1);
        count_row(img, t768, w0, w1, c, 1, r, sink, acc);
    }
}

// The workgroup's findings: lanes -> three LDS words -> one lane's global atomics (a lane per workgroup, not per wave).
__device__ __forceinline__ void rep_init(unsigned long long *rep) {
    if (threadIdx.x < 3) rep[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
}
__device__ __forceinline__ void rep_collect(unsigned long long *rep, const Findings &acc) {
    if (acc.lookups) atomicAdd(rep, (unsigned long long)acc.lookups);
    if (acc.misses) { atomicAdd(rep + 1, (unsigned long long)acc.misses); atomicMin(rep + 2, (unsigned long long)acc.first); }
}
__device__ __forceinline__ void rep_flush(uint64_t *report, const unsigned long long *rep) {  // after __syncthreads()
    if (threadIdx.x == 0) { report_add(report, rep[0]); report_add(report + 1, rep[1]); report_min(report + 2, rep[2]); }
}
__device__ __forceinline__ void load_t768(uint32_t *t768w, const uint8_t *tab768) {
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) t768w[i] = reinterpret_cast<const uint32_t *>(tab768)[i];
}

// A workgroup that counts into LDS: as many waves as the LDS next to the counters holds images for
template <int LAYOUT>
struct CounterGeo {
    static constexpr int LDS = 160 * 1024, FIXED = (int)MULT_COUNTERS * 4 + 768 + 3 * 8;
    static constexpr int WAVES = (LDS - FIXED) / ChkLayout<LAYOUT>::BI >= 8 ? 8 : (LDS - FIXED) / ChkLayout<LAYOUT>::BI;
    static_assert(WAVES >= 4, "a workgroup of at least four waves");
};

// `threads` below: the kernel's blockDim.x, read in the kernel (read in a function here it is loaded the long way round).
// `n` counters added to out[0 .. n): lane i of an instruction adds word i of 64 consecutive ones; zeros are skipped.
__device__ __forceinline__ void flush_add(uint32_t *out, const uint32_t *cnt, uint32_t n, uint32_t threads) {
    for (uint32_t i = threadIdx.x; i < n; i += threads) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}
// The bins `half` of a pair owns, added to the histogram `out` of its set, after __syncthreads(); half 0 reports.
// (The ranges are aesw_mult.h's, taken as constants: the Xor range of half 1 lies a constant stride behind half 0's.)
__device__ __forceinline__ void flush_pair_add(uint32_t *out, const uint32_t *cnt, uint32_t half, uint64_t *report, const unsigned long long *rep, uint32_t threads) {
    constexpr MultFlushRange xr = mult_flush_range(0, 0), xr1 = mult_flush_range(1, 0), low = mult_flush_range(0, 1), high = mult_flush_range(0, 2);
    static_assert(xr1.counter == xr.counter && xr1.length == xr.length, "the two Xor halves differ in their first bin alone");
    flush_add(out + xr.bin + half * (xr1.bin - xr.bin), cnt + xr.counter, xr.length, threads);
    if (half == 0) {
        flush_add(out + low.bin, cnt + low.counter, low.length, threads);
        flush_add(out + high.bin, cnt + high.counter, high.length, threads);
        rep_flush(report, rep);
    }
}

// `words` histogram words to zero and the report to (0 lookups, 0 misses, no miss), by a whole grid: the body of a kernel node,
// not memset nodes, so that a captured graph replays it as it runs eagerly.
__device__ __forceinline__ void zero_and_reset(uint32_t *mult, uint64_t words, uint64_t *report, uint32_t threads) {
    const uint64_t tid = (uint64_t)blockIdx.x * threads + threadIdx.x, n = (uint64_t)gridDim.x * threads;
    report_reset(report, 3, 1u << 2, tid);
    const u32x4 zero = {0, 0, 0, 0};
    for (uint64_t i = tid; i < words / 4; i += n) reinterpret_cast<u32x4 *>(mult)[i] = zero;
    if (tid < words % 4) mult[words - 1 - tid] = 0;
}

}  // namespace multdev
}  // namespace aesw
