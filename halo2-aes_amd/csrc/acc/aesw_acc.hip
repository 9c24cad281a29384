// acc/aesw_acc.hip -- libaesw_acc.so (include/aesw_acc.h): the lookup multiplicities of ONE circuit, accumulated over any
// number of calls, each of which adds a contiguous run of the circuit's blocks.  The bin rule and the sizes
// of the counter split are aesw_mult.h's, the set of a block Placement's, and the counting of a staged unit -- row entries,
// the sinks (and with the LDS one which workgroup of a pair owns which bin), block staging, the
// workgroup's report, the wave count next to the LDS counters -- aesw_mult_dev.h's, shared with libaesw_mult.so.  What is
// here:
//   * acc_reset_kernel: the histograms to zero, the report to (0, 0, none);
//   * acc_add_kernel<LAYOUT>: the run is cut at the set boundaries and every piece into chunks of `chunk` blocks; a pair of
//     workgroups owns a chunk, each counts the bins of its half in LDS and ADDS them to the histogram of the set: lane i of a
//     flush instruction adds bin base + i, a wave 64 consecutive words, a bin that stayed zero is skipped.  Integer adds
//     commute, so the histograms do not depend on how the run was cut, on the order of the calls or on which workgroup arrives
//     first;
//   * acc_key_kernel<LAYOUT>: the 400 rows of one key slab by one wave, one global add per hit (not a hot path);
// and the entry points: their checks, the pieces of a run, the default chunk, the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_acc.h"
#include "../aesw_ctx.h"
#include "../aesw_mult_dev.h"
#include "../aesw_placement.h"

namespace aesw_acc {
using namespace aesw;
using namespace aesw::multdev;

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

// `n` counters added to out[0 .. n): lane i of an instruction adds word i of 64 consecutive ones; zeros are skipped.
__device__ __forceinline__ void flush_add(uint32_t *out, const uint32_t *cnt, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}

// grid: x = 2 * (chunks of the longest piece), y = the pieces (one per set the run touches)
template <int LAYOUT>
__global__ void __launch_bounds__(CounterGeo<LAYOUT>::WAVES * LANES) acc_add_kernel(const RunParams a) {
    using G = ChkLayout<LAYOUT>;
    constexpr int WAVES = CounterGeo<LAYOUT>::WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MULT_COUNTERS];
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
    for (uint32_t i = threadIdx.x; i < MULT_COUNTERS / 4; i += blockDim.x) reinterpret_cast<u32x4 *>(s_cnt)[i] = zero;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    BlockRows rows;
    rows.load(a.table, lane);
    __syncthreads();
    LdsSink sink{s_cnt, half};
    Findings acc;
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
    // (the ranges are aesw_mult.h's, taken as constants: the Xor range of half 1 lies a constant stride behind half 0's)
    constexpr MultFlushRange xr = mult_flush_range(0, 0), xr1 = mult_flush_range(1, 0), low = mult_flush_range(0, 1), high = mult_flush_range(0, 2);
    static_assert(xr1.counter == xr.counter && xr1.length == xr.length, "the two Xor halves differ in their first bin alone");
    flush_add(out + xr.bin + half * (xr1.bin - xr.bin), s_cnt + xr.counter, xr.length);
    if (half == 0) {
        flush_add(out + low.bin, s_cnt + low.counter, low.length);
        flush_add(out + high.bin, s_cnt + high.counter, high.length);
        rep_flush(a.report, s_rep);
    }
}

// One wave: kx | ky | kz into its image, the 400 rows into histogram 0 as unit 0.
template <int LAYOUT>
__global__ void __launch_bounds__(LANES) acc_key_kernel(const KeySlabParams a) {
    using G = ChkLayout<LAYOUT>;
    __shared__ __attribute__((aligned(16))) uint8_t s_img[(G::O_W + 15) / 16 * 16];
    __shared__ uint32_t s_t768[768 / 4];
    const uint32_t lane = threadIdx.x;
    load_t768(s_t768, a.tab768);
    constexpr int KZV = G::KZS % 16 == 0 ? 16 : 8;  // a packed kz is 200 bytes
    Staged<G::KXS, 16> kx; Staged<G::KYS, 16> ky; Staged<G::KZS, KZV> kz;
    kx.load(a.kx, lane); ky.load(a.ky, lane); kz.load(a.kz, lane);
    kx.store(s_img, lane); ky.store(s_img + G::O_KY, lane); kz.store(s_img + G::O_KZ, lane);
    wave_lds_sync();
    GlobalSink sink{a.mult};
    Findings acc;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
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
    if (with_k && !mult_k_ok(k)) return "k must be 2 ... 30";
    if (!mult_sets_ok(n_sets)) return "n_sets must be 1 ... 1024";
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
    if (layout == AESW_LAYOUT_DENSE) hipLaunchKernelGGL((acc_add_kernel<DENSE>), grid, dim3(CounterGeo<DENSE>::WAVES * LANES), 0, s, p);
    else hipLaunchKernelGGL((acc_add_kernel<PACKED>), grid, dim3(CounterGeo<PACKED>::WAVES * LANES), 0, s, p);
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
    if (!mult_has_key_rows(k)) return AESW_OK;
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
