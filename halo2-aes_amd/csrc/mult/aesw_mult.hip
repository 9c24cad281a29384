// mult/aesw_mult.hip -- libaesw_mult.so (include/aesw_mult.h): the lookup multiplicities of a many-circuit batch, one
// histogram of AESW_TABLE_ROWS bins per (circuit, column set).  (A directory of its own, as it is a library of its own: csrc/
// itself holds the sources of libaesw.so.)  The bin rule is aesw_mult.h's, the set of a block Placement's, the tag and the cell
// offsets of a row the check table's (aesw_check.h, uploaded by aesw_create), and the way a slab travels -- 16-byte loads into
// registers, issued for the next block before the current one is walked out of the wave's LDS image -- aesw_check_dev.h's.
// What is here is the scatter, in two forms that give the same bytes:
//   * DIRECT: d_mult is zeroed by a launch of its own; workgroups of four waves share a circuit's blocks, and every hit is one
//     global atomic add into the histogram of the block's set;
//   * PRIVATE: two workgroups own one (circuit, set).  Both walk every block of the set; workgroup 0 counts the Xor rows with
//     x < 128 and the four small sections, workgroup 1 the Xor rows with x >= 128 -- 32 768 (+ 1 024) 32-bit counters in LDS,
//     ds_add -- and each stores its half of the bins once, with plain contiguous stores: no global atomic touches d_mult, and
//     nothing has to zero it first.
// A lane keeps the table entries of its 22 rows in registers for the whole launch: the LDS that is left next to 132 KB of
// counters holds the waves' block images and the 768 table bytes, nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_mult.h"
#include "../aesw_check_dev.h"
#include "../aesw_ctx.h"
#include "../aesw_mult.h"

namespace aesw_mult {
using namespace aesw;

struct MultParams {
    const uint8_t *x, *y, *z;     // the batch's block slabs
    const uint8_t *kx, *ky, *kz;  // n_circuits key slabs: all three, or all null (no key lookups)
    const uint32_t *table;        // build_check_table(layout)
    const uint8_t *tab768;        // sbox | mul2 | mul3
    const uint64_t *offsets;      // n_circuits + 1 (device)
    uint32_t *mult;               // [n_circuits][n_sets][MULT_BINS]
    uint64_t *report;             // aesw_mult_report as 3 x u64
    Placement place;
    uint64_t cap;                 // place.total(n_sets)
    uint32_t n_sets, n_circuits;
    uint32_t groups;              // DIRECT: workgroups per circuit
};

// What one lane found: enabled lookups, misses and the smallest miss (CheckAcc's key, kind CHK_LOOKUP).
struct MultAcc {
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
                                          uint32_t row, Sink &sink, MultAcc &acc) {
    const uint32_t tag = w1 >> 16;
    const uint32_t x = img[w0 & 0xffffu], y = img[w0 >> 16], z = img[w1 & 0xffffu];
    const bool enabled = tag != 0, hit = mult_hit(tag, x, y, z, t768), miss = enabled && !hit;
    acc.lookups += enabled;
    acc.misses += miss;
    const uint64_t key = unit << 20 | (uint64_t)(is_key << 19 | (uint32_t)CHK_LOOKUP << 16 | row);
    acc.first = miss && key < acc.first ? key : acc.first;
    sink.add(hit, tag, x, y);
}

// DIRECT: one global atomic add per hit (no return value: nothing waits for it)
struct GlobalSink {
    uint32_t *hist;  // of the unit's (circuit, set)
    __device__ __forceinline__ void add(bool hit, uint32_t tag, uint32_t x, uint32_t y) {
        if (hit) atomicAdd(hist + mult_bin(tag, x, y), 1u);
    }
};
// PRIVATE: the workgroup's counters.  half 0: Xor rows 512 .. 33 279 and the small sections (U8, Sbox | GfMul2, GfMul3 as 1 024
// consecutive counters); half 1: Xor rows 33 280 .. 66 047.
constexpr uint32_t XOR_FIRST = mult_section_first(2), XOR_HALF = mult_section_rows(2) / 2, SMALL = 4 * 256, SMALL_LOW = 2 * 256;
static_assert(XOR_FIRST == SMALL_LOW && mult_section_first(4) == XOR_FIRST + 2 * XOR_HALF && MULT_ZERO_ROW == mult_section_first(4) + SMALL_LOW,
              "two small sections in front of the Xor section, two behind it");
struct LdsSink {
    uint32_t *cnt;  // XOR_HALF counters of the Xor half, then the SMALL ones
    uint32_t half;
    __device__ __forceinline__ void add(bool hit, uint32_t tag, uint32_t x, uint32_t y) {  // one predicated ds_add, no branch on the tag
        const uint32_t bin = mult_bin(tag, x, y);
        const bool is_xor = tag == 2;
        const uint32_t at = is_xor ? bin - XOR_FIRST - half * XOR_HALF : XOR_HALF + (bin < XOR_FIRST ? bin : bin - 2 * XOR_HALF);
        if (hit && (is_xor ? (x >> 7) == half : half == 0)) atomicAdd(cnt + at, 1u);
    }
};

template <int LAYOUT>
struct BlockStage {
    using G = ChkLayout<LAYOUT>;
    Staged<G::SX, 16> sx; Staged<G::SY, 16> sy; Staged<G::SZ, 16> sz;
    __device__ __forceinline__ void load(const MultParams &a, uint64_t b, uint32_t lane) {
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
    __device__ __forceinline__ void count(const uint8_t *img, const uint8_t *t768, uint64_t b, uint32_t lane, Sink &sink, MultAcc &acc) const {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) count_row(img, t768, w0[j], w1[j], b, 0, lane + LANES * j, sink, acc);
    }
};

// Key slab c by one wave: kx | ky | kz into the wave's image (it is smaller than a block's), its 400 rows into the sink.
template <int LAYOUT, class Sink>
__device__ __forceinline__ void count_key_slab(const MultParams &a, uint32_t c, uint8_t *img, const uint8_t *t768, uint32_t lane, Sink &sink,
                                               MultAcc &acc) {
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
    wave_lds_sync();  // a block overwrites the image
}

// The blocks a circuit places: its count clamped to the capacity, whatever the offsets hold.
__device__ __forceinline__ uint64_t placed_blocks(const MultParams &a, uint32_t c, uint64_t &o0) {
    o0 = a.offsets[c];
    const uint64_t o1 = a.offsets[c + 1];
    return o1 > o0 ? (o1 - o0 < a.cap ? o1 - o0 : a.cap) : 0;
}

// The workgroup's findings: lanes -> three LDS words -> one lane's global atomics (a lane per workgroup, not per wave).
__device__ __forceinline__ void rep_init(unsigned long long *rep) {
    if (threadIdx.x < 3) rep[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
}
__device__ __forceinline__ void rep_collect(unsigned long long *rep, const MultAcc &acc) {
    if (acc.lookups) atomicAdd(rep, (unsigned long long)acc.lookups);
    if (acc.misses) { atomicAdd(rep + 1, (unsigned long long)acc.misses); atomicMin(rep + 2, (unsigned long long)acc.first); }
}
__device__ __forceinline__ void rep_flush(uint64_t *report, const unsigned long long *rep) {  // after __syncthreads()
    if (threadIdx.x == 0) { report_add(report, rep[0]); report_add(report + 1, rep[1]); report_min(report + 2, rep[2]); }
}
__device__ __forceinline__ void load_t768(uint32_t *t768w, const uint8_t *tab768) {
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) t768w[i] = reinterpret_cast<const uint32_t *>(tab768)[i];
}

constexpr int DIRECT_WAVES = 4;
template <int LAYOUT>
__global__ void __launch_bounds__(DIRECT_WAVES * LANES) mult_direct_kernel(const MultParams a) {
    using G = ChkLayout<LAYOUT>;
    __shared__ __attribute__((aligned(16))) uint8_t s_img[DIRECT_WAVES * G::BI];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    const uint32_t c = blockIdx.x / a.groups, g = blockIdx.x - c * a.groups;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    uint8_t *img = s_img + wave * G::BI;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    BlockRows rows;
    rows.load(a.table, lane);
    __syncthreads();
    uint64_t o0;
    const uint64_t n_c = placed_blocks(a, c, o0);
    uint32_t *const circuit = a.mult + (uint64_t)c * a.n_sets * MULT_BINS;
    GlobalSink sink{circuit};
    MultAcc acc;
    if (g == 0 && wave == 0 && a.kx) count_key_slab<LAYOUT>(a, c, img, t768, lane, sink, acc);  // into set 0
    const uint64_t first = (uint64_t)g * DIRECT_WAVES + wave, step = (uint64_t)a.groups * DIRECT_WAVES;
    BlockStage<LAYOUT> st;
    if (first < n_c) st.load(a, o0 + first, lane);
    for (uint64_t j = first; j < n_c; j += step) {
        st.store(img, lane);
        wave_lds_sync();
        if (j + step < n_c) st.load(a, o0 + j + step, lane);  // in flight while this block is counted
        uint32_t set, bi;
        a.place.locate<uint32_t>(j, set, bi);  // j < cap < 2^32; capn > 0 wherever a block is placed
        sink.hist = circuit + (uint64_t)set * MULT_BINS;
        rows.count(img, t768, o0 + j, lane, sink, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    rep_collect(s_rep, acc);
    __syncthreads();
    rep_flush(a.report, s_rep);
}

// PRIVATE: as many waves as the LDS next to the counters holds images for
template <int LAYOUT>
struct PrivateGeo {
    static constexpr int LDS = 160 * 1024, FIXED = (int)(XOR_HALF + SMALL) * 4 + 768 + 3 * 8;
    static constexpr int WAVES = (LDS - FIXED) / ChkLayout<LAYOUT>::BI >= 8 ? 8 : (LDS - FIXED) / ChkLayout<LAYOUT>::BI;
    static_assert(WAVES >= 4, "a workgroup of at least four waves");
};
template <int LAYOUT>
__global__ void __launch_bounds__(PrivateGeo<LAYOUT>::WAVES * LANES) mult_private_kernel(const MultParams a) {
    using G = ChkLayout<LAYOUT>;
    constexpr int WAVES = PrivateGeo<LAYOUT>::WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[XOR_HALF + SMALL];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WAVES * G::BI];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    const uint32_t half = blockIdx.x & 1u, unit = blockIdx.x >> 1;
    const uint32_t c = unit / a.n_sets, set = unit - c * a.n_sets;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    uint8_t *img = s_img + wave * G::BI;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < (XOR_HALF + SMALL) / 4; i += blockDim.x) reinterpret_cast<u32x4 *>(s_cnt)[i] = zero;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    BlockRows rows;
    rows.load(a.table, lane);
    __syncthreads();
    uint64_t o0;
    const uint64_t n_c = placed_blocks(a, c, o0);
    const uint64_t b0 = o0 + a.place.first_block(set), cnt = a.place.filled(set, n_c);
    LdsSink sink{s_cnt, half};
    MultAcc acc;
    if (set == 0 && wave == 0 && a.kx) count_key_slab<LAYOUT>(a, c, img, t768, lane, sink, acc);
    BlockStage<LAYOUT> st;
    if (wave < cnt) st.load(a, b0 + wave, lane);
    for (uint64_t i = wave; i < cnt; i += WAVES) {
        st.store(img, lane);
        wave_lds_sync();
        if (i + WAVES < cnt) st.load(a, b0 + i + WAVES, lane);  // in flight while this block is counted
        rows.count(img, t768, b0 + i, lane, sink, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    if (half == 0) rep_collect(s_rep, acc);  // both workgroups see every row: one of them reports
    __syncthreads();
    // the bins this workgroup owns, each stored once
    uint32_t *const out = a.mult + (uint64_t)unit * MULT_BINS;
    const uint32_t *const s_xor = s_cnt, *const s_small = s_cnt + XOR_HALF;
    if (half == 0) {
        for (uint32_t i = threadIdx.x; i < SMALL_LOW; i += blockDim.x) out[i] = s_small[i];
        for (uint32_t i = threadIdx.x; i < XOR_HALF; i += blockDim.x) out[XOR_FIRST + i] = s_xor[i];
        for (uint32_t i = threadIdx.x; i < SMALL_LOW; i += blockDim.x) out[XOR_FIRST + 2 * XOR_HALF + i] = s_small[SMALL_LOW + i];
        if (threadIdx.x == 0) out[MULT_ZERO_ROW] = 0;
        rep_flush(a.report, s_rep);
    } else {
        for (uint32_t i = threadIdx.x; i < XOR_HALF; i += blockDim.x) out[XOR_FIRST + XOR_HALF + i] = s_xor[i];
    }
}

// The report starts as (0 lookups, 0 misses, no miss), and for the DIRECT form d_mult as zeros: a kernel node, not memset nodes,
// so a captured graph replays it as it runs eagerly.  words == 0: the report alone.
__global__ void __launch_bounds__(256) mult_init_kernel(uint32_t *mult, uint64_t words, uint64_t *report) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n = (uint64_t)gridDim.x * blockDim.x;
    if (tid < 3) report[tid] = tid == 2 ? ~0ull : 0ull;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint64_t i = tid; i < words / 4; i += n) reinterpret_cast<u32x4 *>(mult)[i] = zero;
    if (tid < words % 4) mult[words - 1 - tid] = 0;
}

static hipError_t launch_count(const MultParams &p0, bool dense, int form, hipStream_t s) {
    MultParams p = p0;
    const uint64_t units = (uint64_t)p.n_circuits * p.n_sets, words = form == AESW_MULT_FORM_DIRECT ? units * MULT_BINS : 0;
    const uint64_t zero_groups = (words / 4 + 1023) / 1024;  // four 16-byte stores per lane
    hipLaunchKernelGGL(mult_init_kernel, dim3((unsigned)(zero_groups < 1 ? 1 : zero_groups > 65536 ? 65536 : zero_groups)), dim3(256), 0, s, p.mult, words,
                       p.report);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (form == AESW_MULT_FORM_DIRECT) {
        // a circuit's blocks over up to 64 workgroups of four waves
        const uint64_t g = (p.cap + DIRECT_WAVES - 1) / DIRECT_WAVES;
        p.groups = (uint32_t)(g < 1 ? 1 : g > 64 ? 64 : g);
        const dim3 grid(p.n_circuits * p.groups), block(DIRECT_WAVES * LANES);
        if (dense) hipLaunchKernelGGL((mult_direct_kernel<DENSE>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mult_direct_kernel<PACKED>), grid, block, 0, s, p);
    } else {
        const dim3 grid((unsigned)(2 * units));
        if (dense) hipLaunchKernelGGL((mult_private_kernel<DENSE>), grid, dim3(PrivateGeo<DENSE>::WAVES * LANES), 0, s, p);
        else hipLaunchKernelGGL((mult_private_kernel<PACKED>), grid, dim3(PrivateGeo<PACKED>::WAVES * LANES), 0, s, p);
    }
    return hipGetLastError();
}

// Shape alone decides.  PRIVATE moves the fewest bytes -- every bin is stored once, nothing is zeroed first, no global atomic --
// but has only two workgroups per (circuit, set): below half a chip's worth of them (256 CUs) the DIRECT form, which spreads a
// circuit's blocks over up to 64 workgroups, keeps the chip busy.  k does not enter.
constexpr uint64_t PRIVATE_MIN_WORKGROUPS = 128;
static int default_form(uint32_t /*k*/, uint32_t n_sets, uint32_t n_circuits) {
    return 2 * (uint64_t)n_circuits * n_sets >= PRIVATE_MIN_WORKGROUPS ? AESW_MULT_FORM_PRIVATE : AESW_MULT_FORM_DIRECT;
}

static int refuse(aesw_ctx *ctx, const char *why) {
    if (ctx) ctx->last_error = std::string("aesw_mult_count_device: ") + why;
    return AESW_ERR_INVALID_ARG;
}

}  // namespace aesw_mult

extern "C" {

int aesw_mult_count_device_form(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, int layout,
                                const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slabs, uint32_t *d_mult,
                                aesw_mult_report *d_report, void *stream, int form) {
    using aesw_mult::refuse;
    static_assert(sizeof(aesw_mult_report) == 3 * sizeof(uint64_t), "the kernels address the report as three u64");
    // A histogram counts rows of one set, and a set has 2^k rows: with k <= MAX_K every count fits the 32 bits of a bin (and of
    // an LDS counter), identical blocks included.
    constexpr uint32_t MAX_K = 30, MAX_UNITS = 1u << 24;
    static_assert(MAX_K < 32, "a bin holds 2^k");
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_mult_count_device");
    if (!ctx) return AESW_ERR_INVALID_ARG;
    if (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED) return refuse(ctx, "the layout must be DENSE or PACKED (a VALUES witness has no x)");
    if (k < 2 || k > MAX_K) return refuse(ctx, "k must be 2 ... 30");
    if (n_sets == 0 || n_sets > 1024 || n_circuits == 0 || (uint64_t)n_circuits * n_sets > MAX_UNITS)
        return refuse(ctx, "n_sets must be 1 ... 1024, n_circuits >= 1 and n_circuits * n_sets <= 2^24");
    if (form != AESW_MULT_FORM_AUTO && form != AESW_MULT_FORM_DIRECT && form != AESW_MULT_FORM_PRIVATE) return refuse(ctx, "no such form");
    if (!d_offsets || !aligned_to(d_offsets, 8) || !d_report || !aligned_to(d_report, 8)) return refuse(ctx, "d_offsets and d_report must be there and 8-byte aligned");
    if (!d_mult || !aligned_to(d_mult, 16)) return refuse(ctx, "d_mult must be there and 16-byte aligned");
    if (!d_x || !d_y || !d_z || !aligned_to(d_x, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16))
        return refuse(ctx, "d_x, d_y and d_z must be there and 16-byte aligned");
    const aesw_key_slab *ks = d_key_slabs;
    // a circuit of fewer than KEY_ROWS rows has no room for the key schedule: no key selector is enabled there (aesw_assemble_selectors)
    const bool with_keys = ks && ks->kx && ks->ky && ks->kz && ((uint64_t)1 << k) >= aesw::KEY_ROWS;
    if (with_keys && (!aligned_to(ks->kx, 16) || !aligned_to(ks->ky, 16) || !aligned_to(ks->kz, 16))) return refuse(ctx, "the key columns must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    aesw_mult::MultParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    if (with_keys) { p.kx = ks->kx; p.ky = ks->ky; p.kz = ks->kz; }
    p.table = ctx->d_chktab[layout == AESW_LAYOUT_DENSE ? 0 : 1];  // uploaded by aesw_create(): nothing is allocated here
    p.tab768 = ctx->d_tables;
    p.offsets = d_offsets;
    p.mult = d_mult;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.place = aesw::Placement(k);
    p.cap = p.place.total(n_sets);
    p.n_sets = n_sets;
    p.n_circuits = n_circuits;
    if (form == AESW_MULT_FORM_AUTO) form = aesw_mult::default_form(k, n_sets, n_circuits);
    HIP_TRY(ctx, aesw_mult::launch_count(p, layout == AESW_LAYOUT_DENSE, form, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

int aesw_mult_count_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, int layout,
                           const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slabs, uint32_t *d_mult,
                           aesw_mult_report *d_report, void *stream) {
    return aesw_mult_count_device_form(ctx, k, n_sets, n_circuits, d_offsets, layout, d_x, d_y, d_z, d_key_slabs, d_mult, d_report, stream,
                                       AESW_MULT_FORM_AUTO);
}

int aesw_mult_default_form(uint32_t k, uint32_t n_sets, uint32_t n_circuits) { return aesw_mult::default_form(k, n_sets, n_circuits); }

uint32_t aesw_mult_bin(uint32_t tag, uint32_t x, uint32_t y) { return aesw::mult_bin(tag, x, y); }

}  // extern "C"
