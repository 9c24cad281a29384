// vacc/aesw_vacc.hip -- libaesw_vacc.so (include/aesw_vacc.h): the lookups of a run of ONE circuit's blocks, given as a VALUES
// witness, added to the histograms of libaesw_acc.so.  The bin rule and the counter split are aesw_mult.h's, the
// set of a block Placement's, the run -- its pieces, its chunks, the grid, the default chunk -- aesw_run.h's, the counting of a
// row, the sinks, the findings, the workgroup's report, the add flush of a pair and the checks of the outputs aesw_mult_dev.h's,
// and which cell an operand of a lookup is aesw_vals_check.h's, rebased onto the image of aesw_vacc.h.  What is here:
//   * vacc_count_kernel: acc_add_kernel's division of labour -- the run cut at the set boundaries, every piece into chunks, a
//     pair of workgroups per chunk, each counting the bins of its half in LDS and ADDING them to the histogram of the set -- over
//     a block's 448 y + 608 z + 16 plaintext bytes and the circuit's 176 round-key cells: 17 row steps per lane, no x column;
//   * the table, in the code object's own storage, filled once per device;
//   * the entry points: the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's) and the launch.
// The reset and the key slab's own 400 rows are libaesw_acc.so's (the key slabs of VALUES are the packed ones): nothing of them
// is restated here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../../include/aesw_vacc.h"
#include "../aesw_entry.h"
#include "../aesw_mult_dev.h"
#include "../aesw_run.h"
#include "../aesw_vacc.h"

namespace aesw_vacc {
using namespace aesw;
using namespace aesw::multdev;

// The waves of a workgroup.  Next to the counters the LDS holds 20 images of VACC_IMG bytes, so registers decide, not LDS: 8 is
// acc_add_kernel<PACKED>'s count; 16 is the other candidate tools/vacc_bench.py builds and times (DESIGN 4.17 has the figures).
#ifndef AESW_VACC_WAVES
#define AESW_VACC_WAVES 8
#endif
constexpr int WAVES = AESW_VACC_WAVES;
constexpr int ROW_STEPS = (VALS_ROWS + LANES - 1) / LANES;  // 17 entries per lane (1 056 = 16.5 x 64)
static_assert(WAVES >= 4 && WAVES <= 16 && (int)MULT_COUNTERS * 4 + 768 + 3 * 8 + WAVES * VACC_IMG <= 160 * 1024, "counters, tab768, report and the images fit the LDS");

struct RunParams {
    const uint8_t *pt, *y, *z;  // of circuit blocks [first, end): block first + i at pt + 16 i, y + 448 i, z + 608 i
    const uint8_t *kz, *kw;     // the circuit's packed key slab: kz (200 bytes) and words_column (96)
    const uint32_t *table;      // build_vacc_table
    const uint8_t *tab768;      // sbox | mul2 | mul3
    uint32_t *mult;             // [n_sets][MULT_BINS]
    uint64_t *report;           // aesw_mult_report as 3 x u64
    Run run;
};

// The table of this library, one copy per device, filled by ensure_table().
__device__ uint32_t g_vacc_table[VACC_WORDS];

// A block on its way into the wave's image: y and z as 16-byte units, the plaintext as one 16-byte load of lane 0.
struct ValuesStage {
    Staged<Geo<VALUES>::YS, 16> sy; Staged<Geo<VALUES>::ZS, 16> sz;
    u32x4 pt = {0, 0, 0, 0};
    __device__ __forceinline__ void load(const RunParams &a, uint64_t b, uint32_t lane) {
        sy.load(a.y + b * Geo<VALUES>::YS, lane); sz.load(a.z + b * Geo<VALUES>::ZS, lane);
        if (lane == 0) pt = *reinterpret_cast<const u32x4 *>(a.pt + b * 16);
    }
    __device__ __forceinline__ void store(uint8_t *img, uint32_t lane) const {
        sy.store(img, lane); sz.store(img + VALS_O_Z, lane);
        if (lane == 0) *reinterpret_cast<u32x4 *>(img + VALS_O_PT) = pt;
    }
};
static_assert(Geo<VALUES>::YS == VALS_O_Z && VALS_O_Z + Geo<VALUES>::ZS == VALS_O_PT, "y | z | pt");

// The lane's entries lane + 64 j, read once.  Past entry 1 055: tag 0, no lookup.  A finding is keyed by the ENTRY, a constant of
// the unrolled step: entries are in slab-row order (build_vacc_table checks it), so the smallest key names the smallest slab row,
// and the one that is left at the end is translated once (first_to_slab_row) -- no register holds a slab row.
struct ValuesRows {
    uint32_t w0[ROW_STEPS], w1[ROW_STEPS];
    __device__ __forceinline__ void load(const uint32_t *table, uint32_t lane) {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) {
            const uint32_t e = lane + LANES * j;
            w0[j] = w1[j] = 0;
            if (e < (uint32_t)VALS_ROWS) row_entry(table, 2 * e, 0, w0[j], w1[j]);
        }
    }
    template <class Sink>
    __device__ __forceinline__ void count(const uint8_t *img, const uint8_t *t768, uint64_t b, uint32_t lane, Sink &sink, Findings &acc) const {
#pragma unroll
        for (int j = 0; j < ROW_STEPS; ++j) count_row(img, t768, w0[j], w1[j], b, 0, lane + LANES * j, sink, acc);
    }
};
__device__ __forceinline__ void first_to_slab_row(const uint32_t *table, Findings &acc) {
    if (acc.first != ~0ull) acc.first = (acc.first & ~0xffffull) | vacc_slab_row(table, (uint32_t)(acc.first & 0xffffu));
}

// grid: x = 2 * (chunks of the longest piece), y = the pieces (one per set the run touches)
__global__ void __launch_bounds__(WAVES * LANES) vacc_count_kernel(const RunParams a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MULT_COUNTERS];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WAVES * VACC_IMG];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const auto [half, set, b0, cnt] = a.run.chunk_at(blockIdx.x, blockIdx.y);
    if (cnt == 0) return;  // the whole workgroup: a shorter piece than the longest one
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    uint8_t *img = s_img + wave * VACC_IMG;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < MULT_COUNTERS / 4; i += blockDim.x) reinterpret_cast<u32x4 *>(s_cnt)[i] = zero;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    ValuesRows rows;
    rows.load(a.table, lane);
    {  // the round-key cells do not change from block to block: once per wave, behind the block image
        Staged<VALS_ST.kz, 8> kz; Staged<WORDS_ROWS, 8> kw;
        kz.load(a.kz, lane); kw.load(a.kw, lane);
        kz.store(img + VACC_O_KZ, lane); kw.store(img + VACC_O_W, lane);
    }
    __syncthreads();
    LdsSink sink{s_cnt, half};
    Findings acc;
    ValuesStage st;
    if (wave < cnt) st.load(a, b0 + wave - a.run.first, lane);
    for (uint64_t i = wave; i < cnt; i += WAVES) {
        st.store(img, lane);
        wave_lds_sync();
        if (i + WAVES < cnt) st.load(a, b0 + i + WAVES - a.run.first, lane);  // in flight while this block is counted
        rows.count(img, t768, b0 + i, lane, sink, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    if (half == 0) {  // both workgroups see every row: one of them reports
        first_to_slab_row(a.table, acc);
        rep_collect(s_rep, acc);
    }
    __syncthreads();
    flush_pair_add(a.mult + (uint64_t)set * MULT_BINS, s_cnt, half, a.report, s_rep, blockDim.x);
}

// The table lives in the code object's own storage: nothing to allocate, nothing to free.  It is filled once per
// device and process; the copy is synchronous, and legal while some stream of this thread is being captured (relaxed capture
// mode for the length of the copy).  Called with the context's device current.
constexpr int MAX_DEVICES = 64;
static int ensure_table(aesw_ctx *ctx, const uint32_t **d_table) {
    static std::mutex mu;
    static const uint32_t *uploaded[MAX_DEVICES] = {};
    if (ctx->device < 0 || ctx->device >= MAX_DEVICES) return AESW_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(mu);
    if (!uploaded[ctx->device]) {
        std::vector<uint32_t> host(VACC_WORDS);
        if (build_vacc_table(host.data()) != 0) {
            ctx->last_error = "aesw_vacc: an operand of a block's lookups does not lie in the counting image";
            return AESW_ERR_INVALID_ARG;
        }
        void *p = nullptr;
        HIP_TRY(ctx, hipGetSymbolAddress(&p, HIP_SYMBOL(g_vacc_table)));
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        HIP_TRY(ctx, hipThreadExchangeStreamCaptureMode(&mode));
        const hipError_t e = hipMemcpy(p, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        (void)hipThreadExchangeStreamCaptureMode(&mode);
        HIP_TRY(ctx, e);
        uploaded[ctx->device] = static_cast<const uint32_t *>(p);
    }
    *d_table = uploaded[ctx->device];
    return AESW_OK;
}

}  // namespace aesw_vacc

extern "C" {

int aesw_vacc_add_device_chunk(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, const uint8_t *d_pt,
                               const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slab, uint32_t *d_mult,
                               aesw_mult_report *d_report, void *stream, uint32_t blocks_per_workgroup) {
    using namespace aesw_vacc;
    static_assert(sizeof(aesw_mult_report) == 3 * sizeof(uint64_t), "the kernel addresses the report as three u64");
    const char *const call = "aesw_vacc_add_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_outputs(k, true, n_sets, d_mult, d_report)) return refuse(ctx, call, why);
    const Placement place(k);
    const uint64_t cap = place.total(n_sets);
    if (first_block > cap || n_blocks > cap - first_block)
        return refuse(ctx, call, "first_block + n_blocks is more than aesw_block_capacity(k, n_sets)", AESW_ERR_CAPACITY);
    if (n_blocks == 0) return AESW_OK;
    if (!d_pt || !d_y || !d_z || !aligned_to(d_pt, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16))
        return refuse(ctx, call, "d_pt, d_y and d_z must be there and 16-byte aligned");
    const aesw_key_slab *ks = d_key_slab;
    if (!ks || !ks->kz || !ks->w || !aligned_to(ks->kz, 16) || !aligned_to(ks->w, 16))
        return refuse(ctx, call, "d_key_slab is required: its kz and words_column must be there and 16-byte aligned");
    RunParams p{};
    p.pt = d_pt; p.y = d_y; p.z = d_z;
    p.kz = ks->kz; p.kw = ks->w;
    p.tab768 = ctx->d_tables;
    p.mult = d_mult;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    const RunPlan plan = run_plan(place, first_block, n_blocks, blocks_per_workgroup);
    if (!plan.fits()) return refuse(ctx, call, "blocks_per_workgroup leaves more than 2^22 chunks in one set");
    p.run = plan.run;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const int rc = ensure_table(ctx, &p.table);
    if (rc != AESW_OK) return rc;
    const dim3 grid((unsigned)(2 * plan.pairs), plan.pieces);
    hipLaunchKernelGGL(vacc_count_kernel, grid, dim3(WAVES * LANES), 0, reinterpret_cast<hipStream_t>(stream), p);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_vacc_add_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t first_block, uint64_t n_blocks, const uint8_t *d_pt, const uint8_t *d_y,
                         const uint8_t *d_z, const aesw_key_slab *d_key_slab, uint32_t *d_mult, aesw_mult_report *d_report, void *stream) {
    return aesw_vacc_add_device_chunk(ctx, k, n_sets, first_block, n_blocks, d_pt, d_y, d_z, d_key_slab, d_mult, d_report, stream, 0);
}

uint32_t aesw_vacc_default_chunk(uint32_t /*k*/, uint32_t /*n_sets*/, uint64_t /*first_block*/, uint64_t n_blocks) {
    return aesw::run_default_chunk(n_blocks);
}

int aesw_vacc_prepare(aesw_ctx *ctx) {
    if (int rc = aesw::entry_refused(ctx, "aesw_vacc_prepare")) return rc;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const uint32_t *t = nullptr;
    return aesw_vacc::ensure_table(ctx, &t);
}

}  // extern "C"
