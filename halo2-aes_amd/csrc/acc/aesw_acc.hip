// acc/aesw_acc.hip -- libaesw_acc.so (include/aesw_acc.h): the lookup multiplicities of ONE circuit, accumulated over any number
// of calls, each of which adds a contiguous run of the circuit's blocks.  The bin rule is aesw_mult.h's, the
// set of a block Placement's, the tag and the cell offsets of a row the check table's (aesw_check.h, uploaded by aesw_create),
// and the way a slab travels -- 16-byte loads into registers, issued for the next block before the current one is walked out of
// the wave's LDS image -- aesw_check_dev.h's.  What is here:
//   * acc_reset_kernel: the histograms to zero (16-byte stores), the report to (0, 0, none);
//   * acc_add_kernel<LAYOUT>: the division of labour of mult_private_kernel (mult/aesw_mult.hip) with (set, chunk) in place of
//     (circuit, set).  The run is cut at the set boundaries and every piece into chunks of `chunk` blocks; a pair of workgroups
//     owns a chunk -- workgroup 0 counts the Xor rows with x < 128 and the four small sections, workgroup 1 the Xor rows with
//     x >= 128, in 32-bit LDS counters -- and each ADDS its half to the histogram of the set: lane i of a flush instruction adds
//     bin base + i, a wave 64 consecutive words, a bin that stayed zero is skipped.  Integer adds commute, so the histograms do
//     not depend on how the run was cut, on the order of the calls or on which workgroup arrives first;
//   * acc_key_kernel<LAYOUT>: the 400 rows of one key slab by one wave, one global add per hit (not a hot path).
// The row walk restates the one of mult/aesw_mult.hip: that file is a translation unit, not a header, and moving the walk into
// one would recompile libaesw_mult.so, whose kernels are pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_acc.h"
#include "../aesw_check_dev.h"
#include "../aesw_ctx.h"
#include "../aesw_mult.h"
#include "../aesw_placement.h"

namespace aesw_acc {
using namespace aesw;

struct RunParams {
    const uint8_t *x, *y, *z;  // the slabs of circuit blocks [first, end): slab i is block first + i
    const uint32_t *table;     // build_check_table(layout)
    const uint8_t *tab768;     // sbox | mul2 | mul3
    uint32_t *mult;            // [n_sets][MULT_BINS]
    uint64_t *report;          // aesw_mult_report as 3 x u64
    Placement place;
    uint64_t first, end;
    uint32_t set0;             // the set of block `first`: blockIdx.y counts the pieces from it
    uint32_t chunk;            // blocks per pair of workgroups
};
struct KeySlabParams {
    const uint8_t *kx, *ky, *kz;
    const uint32_t *table;
    const uint8_t *tab768;
    uint32_t *mult;  // histogram 0
    uint64_t *report;
};

// What one lane found: enabled lookups, misses and the smallest miss (CheckAcc's key, kind CHK_LOOKUP).
struct LaneAcc {
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
                                          uint32_t row, Sink &sink, LaneAcc &acc) {
    const uint32_t tag = w1 >> 16;
    const uint32_t x = img[w0 & 0xffffu], y = img[w0 >> 16], z = img[w1 & 0xffffu];
    const bool enabled = tag != 0, hit = mult_hit(tag, x, y, z, t768), miss = enabled && !hit;
    acc.lookups += enabled;
    acc.misses += miss;
    const uint64_t key = unit << 20 | (uint64_t)(is_key << 19 | (uint32_t)CHK_LOOKUP << 16 | row);
    acc.first = miss && key < acc.first ? key : acc.first;
    sink.add(hit, tag, x, y);
}

// The key rows: one global add per hit (no return value: nothing waits for it)
struct GlobalSink {
    uint32_t *hist;
    __device__ __forceinline__ void add(bool hit, uint32_t tag, uint32_t x, uint32_t y) {
        if (hit) atomicAdd(hist + mult_bin(tag, x, y), 1u);
    }
};
// The blocks: the workgroup's counters.  half 0: Xor rows 512 .. 33 279 and the small sections (U8, Sbox | GfMul2, GfMul3 as
// 1 024 consecutive counters); half 1: Xor rows 33 280 .. 66 047.
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
    __device__ __forceinline__ void load(const RunParams &a, uint64_t slab, uint32_t lane) {
        sx.load(a.x + slab * G::SX, lane); sy.load(a.y + slab * G::SY, lane); sz.load(a.z + slab * G::SZ, lane);
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
    __device__ __forceinline__ void count(const uint8_t *img, const uint8_t *t768, uint64_t b, uint32_t lane, Sink &sink, LaneAcc &acc) const {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) count_row(img, t768, w0[j], w1[j], b, 0, lane + LANES * j, sink, acc);
    }
};

// The workgroup's findings: lanes -> three LDS words -> one lane's global atomics (a lane per workgroup, not per wave).
__device__ __forceinline__ void rep_init(unsigned long long *rep) {
    if (threadIdx.x < 3) rep[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
}
__device__ __forceinline__ void rep_collect(unsigned long long *rep, const LaneAcc &acc) {
    if (acc.lookups) atomicAdd(rep, (unsigned long long)acc.lookups);
    if (acc.misses) { atomicAdd(rep + 1, (unsigned long long)acc.misses); atomicMin(rep + 2, (unsigned long long)acc.first); }
}
__device__ __forceinline__ void rep_flush(uint64_t *report, const unsigned long long *rep) {  // after __syncthreads()
    if (threadIdx.x == 0) { report_add(report, rep[0]); report_add(report + 1, rep[1]); report_min(report + 2, rep[2]); }
}
__device__ __forceinline__ void load_t768(uint32_t *t768w, const uint8_t *tab768) {
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) t768w[i] = reinterpret_cast<const uint32_t *>(tab768)[i];
}

// `n` counters added to out[0 .. n): lane i of an instruction adds word i of 64 consecutive ones; zeros are skipped.
__device__ __forceinline__ void flush_add(uint32_t *out, const uint32_t *cnt, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}

// as many waves as the LDS next to the counters holds images for
template <int LAYOUT>
struct AddGeo {
    static constexpr int LDS = 160 * 1024, FIXED = (int)(XOR_HALF + SMALL) * 4 + 768 + 3 * 8;
    static constexpr int WAVES = (LDS - FIXED) / ChkLayout<LAYOUT>::BI >= 8 ? 8 : (LDS - FIXED) / ChkLayout<LAYOUT>::BI;
    static_assert(WAVES >= 4, "a workgroup of at least four waves");
};
// grid: x = 2 * (chunks of the longest piece), y = the pieces (one per set the run touches)
template <int LAYOUT>
__global__ void __launch_bounds__(AddGeo<LAYOUT>::WAVES * LANES) acc_add_kernel(const RunParams a) {
    using G = ChkLayout<LAYOUT>;
    constexpr int WAVES = AddGeo<LAYOUT>::WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[XOR_HALF + SMALL];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WAVES * G::BI];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const uint32_t half = blockIdx.x & 1u, set = a.set0 + blockIdx.y;
    // the piece: the run's blocks in this set; the chunk: `chunk` of them (fewer at the piece's end)
    const uint64_t s_lo = a.place.first_block(set), s_hi = s_lo + a.place.capacity(set);
    const uint64_t lo = a.first > s_lo ? a.first : s_lo, hi = a.end < s_hi ? a.end : s_hi;
    const uint64_t b0 = lo + (uint64_t)(blockIdx.x >> 1) * a.chunk;
    if (b0 >= hi) return;  // the whole workgroup: a shorter piece than the longest one
    const uint64_t cnt = hi - b0 < a.chunk ? hi - b0 : a.chunk;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    uint8_t *img = s_img + wave * G::BI;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < (XOR_HALF + SMALL) / 4; i += blockDim.x) reinterpret_cast<u32x4 *>(s_cnt)[i] = zero;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    BlockRows rows;
    rows.load(a.table, lane);
    __syncthreads();
    LdsSink sink{s_cnt, half};
    LaneAcc acc;
    BlockStage<LAYOUT> st;
    if (wave < cnt) st.load(a, b0 + wave - a.first, lane);
    for (uint64_t i = wave; i < cnt; i += WAVES) {
        st.store(img, lane);
        wave_lds_sync();
        if (i + WAVES < cnt) st.load(a, b0 + i + WAVES - a.first, lane);  // in flight while this block is counted
        rows.count(img, t768, b0 + i, lane, sink, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    if (half == 0) rep_collect(s_rep, acc);  // both workgroups see every row: one of them reports
    __syncthreads();
    // the bins this workgroup owns, added to the set's histogram
    uint32_t *const out = a.mult + (uint64_t)set * MULT_BINS;
    const uint32_t *const s_xor = s_cnt, *const s_small = s_cnt + XOR_HALF;
    flush_add(out + XOR_FIRST + half * XOR_HALF, s_xor, XOR_HALF);
    if (half == 0) {
        flush_add(out, s_small, SMALL_LOW);
        flush_add(out + XOR_FIRST + 2 * XOR_HALF, s_small + SMALL_LOW, SMALL_LOW);
        rep_flush(a.report, s_rep);
    }
}

// One wave: kx | ky | kz into its image, the 400 rows into histogram 0.
template <int LAYOUT>
__global__ void __launch_bounds__(LANES) acc_key_kernel(const KeySlabParams a) {
    using G = ChkLayout<LAYOUT>;
    __shared__ __attribute__((aligned(16))) uint8_t s_img[(G::O_W + 15) / 16 * 16];
    __shared__ uint32_t s_t768[768 / 4];
    constexpr int KZV = G::KZS % 16 == 0 ? 16 : 8;  // a packed kz is 200 bytes
    const uint32_t lane = threadIdx.x;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    load_t768(s_t768, a.tab768);
    Staged<G::KXS, 16> kx; Staged<G::KYS, 16> ky; Staged<G::KZS, KZV> kz;
    kx.load(a.kx, lane); ky.load(a.ky, lane); kz.load(a.kz, lane);
    kx.store(s_img, lane); ky.store(s_img + G::O_KY, lane); kz.store(s_img + G::O_KZ, lane);
    wave_lds_sync();
    GlobalSink sink{a.mult};
    LaneAcc acc;
    for (uint32_t r = lane; r < (uint32_t)KEY_ROWS; r += LANES) {
        uint32_t w0, w1;
        row_entry(a.table, CHK_KROWS + 2 * r, G::BI, w0, w1);
        count_row(s_img, t768, w0, w1, 0, 1, r, sink, acc);
    }
    report_add(a.report, acc.lookups);
    report_add(a.report + 1, acc.misses);
    report_min(a.report + 2, acc.first);
}

// A kernel node, not memset nodes, so that a captured graph replays it as it runs eagerly.
__global__ void __launch_bounds__(256) acc_reset_kernel(uint32_t *mult, uint64_t words, uint64_t *report) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n = (uint64_t)gridDim.x * blockDim.x;
    if (tid < 3) report[tid] = tid == 2 ? ~0ull : 0ull;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint64_t i = tid; i < words / 4; i += n) reinterpret_cast<u32x4 *>(mult)[i] = zero;
    if (tid < words % 4) mult[words - 1 - tid] = 0;
}

// The default chunk, from the shape alone.  A pair of workgroups flushes up to 65 536 + 1 024 words however few
// blocks it counted, so a chunk is at least MIN_CHUNK blocks: 256 x 608 Xor lookups, more than twice the words of the flush,
// and 32 blocks per wave in front of a flush of 66 steps.  Above that the run is spread over TARGET_PAIRS pairs: the counters
// leave room for one workgroup per CU, and 128 pairs are 256 workgroups, one per CU of the chip.
constexpr uint64_t MIN_CHUNK = 256, TARGET_PAIRS = 128, MAX_PAIRS_PER_SET = 1ull << 22;
static uint32_t default_chunk(uint64_t n_blocks) {
    const uint64_t spread = (n_blocks + TARGET_PAIRS - 1) / TARGET_PAIRS;  // n_blocks < 2^30: it fits
    return (uint32_t)(spread < MIN_CHUNK ? MIN_CHUNK : spread);
}

static int refuse(aesw_ctx *ctx, const char *call, const char *why, int status = AESW_ERR_INVALID_ARG) {
    if (ctx) ctx->last_error = std::string(call) + ": " + why;
    return status;
}
// what every call checks of its outputs and of the circuit's shape (with_k: the call takes a k)
static const char *bad_outputs(uint32_t k, bool with_k, uint32_t n_sets, const uint32_t *d_mult, const aesw_mult_report *d_report) {
    if (with_k && (k < 2 || k > 30)) return "k must be 2 ... 30";
    if (n_sets == 0 || n_sets > 1024) return "n_sets must be 1 ... 1024";
    if (!d_report || !aligned_to(d_report, 8)) return "d_report must be there and 8-byte aligned";
    if (!d_mult || !aligned_to(d_mult, 16)) return "d_mult must be there and 16-byte aligned";
    return nullptr;
}

}  // namespace aesw_acc

extern "C" {

int aesw_acc_reset_device(aesw_ctx *ctx, uint32_t n_sets, uint32_t *d_mult, aesw_mult_report *d_report, void *stream) {
    using namespace aesw_acc;
    static_assert(sizeof(aesw_mult_report) == 3 * sizeof(uint64_t), "the kernels address the report as three u64");
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_acc_reset_device");
    if (!ctx) return AESW_ERR_INVALID_ARG;
    if (const char *why = bad_outputs(0, false, n_sets, d_mult, d_report)) return refuse(ctx, "aesw_acc_reset_device", why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const uint64_t words = (uint64_t)n_sets * MULT_BINS, groups = (words / 4 + 1023) / 1024;  // four 16-byte stores per lane
    hipLaunchKernelGGL(acc_reset_kernel, dim3((unsigned)(groups < 1 ? 1 : groups)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_mult, words,
                       reinterpret_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_acc_add_device_chunk(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, int layout,
                              const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, uint32_t *d_mult, aesw_mult_report *d_report,
                              void *stream, uint32_t blocks_per_workgroup) {
    using namespace aesw_acc;
    const char *const call = "aesw_acc_add_device";
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, call);
    if (!ctx) return AESW_ERR_INVALID_ARG;
    if (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED) return refuse(ctx, call, "the layout must be DENSE or PACKED (a VALUES witness has no x)");
    // A histogram counts rows of one set, and a set has 2^k rows: with k <= 30 every count fits the 32 bits of a bin (and of an
    // LDS counter), identical blocks included.
    if (const char *why = bad_outputs(k, true, n_sets, d_mult, d_report)) return refuse(ctx, call, why);
    const Placement place(k);
    const uint64_t cap = place.total(n_sets);
    if (first_block > cap || n_blocks > cap - first_block)
        return refuse(ctx, call, "first_block + n_blocks is more than aesw_block_capacity(k, n_sets)", AESW_ERR_CAPACITY);
    if (n_blocks == 0) return AESW_OK;
    if (!d_x || !d_y || !d_z || !aligned_to(d_x, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16))
        return refuse(ctx, call, "d_x, d_y and d_z must be there and 16-byte aligned");
    RunParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    p.table = ctx->d_chktab[layout == AESW_LAYOUT_DENSE ? 0 : 1];  // uploaded by aesw_create(): nothing is allocated here
    p.tab768 = ctx->d_tables;
    p.mult = d_mult;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.place = place;
    p.first = first_block;
    p.end = first_block + n_blocks;
    p.chunk = blocks_per_workgroup ? blocks_per_workgroup : default_chunk(n_blocks);
    // the pieces: one per set from the first block's to the last block's; the longest one decides the grid's width
    uint32_t set1;
    uint64_t bi;
    place.locate<uint64_t>(first_block, p.set0, bi);
    place.locate<uint64_t>(p.end - 1, set1, bi);
    const auto piece = [&](uint32_t s) {
        const uint64_t s_lo = place.first_block(s), s_hi = s_lo + place.capacity(s);
        return (p.end < s_hi ? p.end : s_hi) - (p.first > s_lo ? p.first : s_lo);
    };
    uint64_t longest = piece(p.set0);
    if (set1 > p.set0 && piece(set1) > longest) longest = piece(set1);
    if (set1 > p.set0 + 1 && piece(p.set0 + 1) > longest) longest = piece(p.set0 + 1);  // every piece between the two is a whole set
    const uint64_t pairs = (longest + p.chunk - 1) / p.chunk;
    if (pairs > MAX_PAIRS_PER_SET) return refuse(ctx, call, "blocks_per_workgroup leaves more than 2^22 chunks in one set");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const dim3 grid((unsigned)(2 * pairs), set1 - p.set0 + 1);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == AESW_LAYOUT_DENSE) hipLaunchKernelGGL((acc_add_kernel<DENSE>), grid, dim3(AddGeo<DENSE>::WAVES * LANES), 0, s, p);
    else hipLaunchKernelGGL((acc_add_kernel<PACKED>), grid, dim3(AddGeo<PACKED>::WAVES * LANES), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_acc_add_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, int layout, const uint8_t *d_x,
                        const uint8_t *d_y, const uint8_t *d_z, uint32_t *d_mult, aesw_mult_report *d_report, void *stream) {
    return aesw_acc_add_device_chunk(ctx, k, n_sets, first_block, n_blocks, layout, d_x, d_y, d_z, d_mult, d_report, stream, 0);
}

int aesw_acc_add_key_device(aesw_ctx *ctx, uint32_t k, int layout, const aesw_key_slab *d_key_slab, uint32_t *d_mult, aesw_mult_report *d_report,
                            void *stream) {
    using namespace aesw_acc;
    const char *const call = "aesw_acc_add_key_device";
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, call);
    if (!ctx) return AESW_ERR_INVALID_ARG;
    if (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED) return refuse(ctx, call, "the layout must be DENSE or PACKED (a VALUES witness has no x)");
    if (const char *why = bad_outputs(k, true, 1, d_mult, d_report)) return refuse(ctx, call, why);
    const aesw_key_slab *ks = d_key_slab;
    if (!ks || !ks->kx || !ks->ky || !ks->kz || !aligned_to(ks->kx, 16) || !aligned_to(ks->ky, 16) || !aligned_to(ks->kz, 16))
        return refuse(ctx, call, "the key columns kx, ky and kz must be there and 16-byte aligned");
    // a circuit of fewer than KEY_ROWS rows has no room for the key schedule: no key selector is enabled there (aesw_assemble_selectors)
    if (((uint64_t)1 << k) < aesw::KEY_ROWS) return AESW_OK;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    KeySlabParams p{};
    p.kx = ks->kx; p.ky = ks->ky; p.kz = ks->kz;
    p.table = ctx->d_chktab[layout == AESW_LAYOUT_DENSE ? 0 : 1];
    p.tab768 = ctx->d_tables;
    p.mult = d_mult;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layout == AESW_LAYOUT_DENSE) hipLaunchKernelGGL((acc_key_kernel<DENSE>), dim3(1), dim3(LANES), 0, s, p);
    else hipLaunchKernelGGL((acc_key_kernel<PACKED>), dim3(1), dim3(LANES), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

uint32_t aesw_acc_default_chunk(uint32_t /*k*/, uint32_t /*n_sets*/, uint64_t /*first_block*/, uint64_t n_blocks) {
    return aesw_acc::default_chunk(n_blocks);
}

}  // extern "C"
