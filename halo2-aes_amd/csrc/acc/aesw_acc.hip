// acc/aesw_acc.hip -- libaesw_acc.so (include/aesw_acc.h): the lookup multiplicities of ONE circuit, accumulated over any
// number of calls, each of which adds a contiguous run of the circuit's blocks.  The bin rule and the sizes
// of the counter split are aesw_mult.h's, the set of a block Placement's, the run -- its pieces, its chunks, the grid, the
// default chunk -- aesw_run.h's, shared with libaesw_vacc.so, and the counting of a staged unit -- row entries, the sinks (and
// with the LDS one which workgroup of a pair owns which bin), block staging, the workgroup's report, the wave count next to the
// LDS counters, the add flush of a pair, the zeroing body, the checks of the outputs -- aesw_mult_dev.h's, shared with
// libaesw_mult.so and libaesw_vacc.so.  What is here:
//   * acc_reset_kernel: the histograms to zero, the report to (0, 0, none) (zero_and_reset under this library's name);
//   * acc_add_kernel<LAYOUT>: the run is cut at the set boundaries and every piece into chunks of `chunk` blocks; a pair of
//     workgroups owns a chunk, each counts the bins of its half in LDS and ADDS them to the histogram of the set: lane i of a
//     flush instruction adds bin base + i, a wave 64 consecutive words, a bin that stayed zero is skipped.  Integer adds
//     commute, so the histograms do not depend on how the run was cut, on the order of the calls or on which workgroup arrives
//     first;
//   * acc_key_kernel<LAYOUT>: the 400 rows of one key slab by one wave, one global add per hit (not a hot path);
// and the entry points: the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's) and the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_acc.h"
#include "../aesw_entry.h"
#include "../aesw_mult_dev.h"
#include "../aesw_run.h"

namespace aesw_acc {
using namespace aesw;
using namespace aesw::multdev;

struct RunParams {
    const uint8_t *x, *y, *z;  // the slabs of circuit blocks [first, end): slab i is block first + i
    const uint32_t *table;     // build_check_table(layout)
    const uint8_t *tab768;     // sbox | mul2 | mul3
    uint32_t *mult;            // [n_sets][MULT_BINS]
    uint64_t *report;          // aesw_mult_report as 3 x u64
    Run run;
};
struct KeySlabParams {
    const uint8_t *kx, *ky, *kz;
    const uint32_t *table;
    const uint8_t *tab768;
    uint32_t *mult;  // histogram 0
    uint64_t *report;
};

// grid: x = 2 * (chunks of the longest piece), y = the pieces (one per set the run touches)
template <int LAYOUT>
__global__ void __launch_bounds__(CounterGeo<LAYOUT>::WAVES * LANES) acc_add_kernel(const RunParams a) {
    using G = ChkLayout<LAYOUT>;
    constexpr int WAVES = CounterGeo<LAYOUT>::WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MULT_COUNTERS];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WAVES * G::BI];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const auto [half, set, b0, cnt] = a.run.chunk_at(blockIdx.x, blockIdx.y);
    if (cnt == 0) return;  // the whole workgroup: a shorter piece than the longest one
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
    if (wave < cnt) st.load(a, b0 + wave - a.run.first, lane);
    for (uint64_t i = wave; i < cnt; i += WAVES) {
        st.store(img, lane);
        wave_lds_sync();
        if (i + WAVES < cnt) st.load(a, b0 + i + WAVES - a.run.first, lane);  // in flight while this block is counted
        rows.count(img, t768, b0 + i, lane, sink, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    if (half == 0) rep_collect(s_rep, acc);  // both workgroups see every row: one of them reports
    __syncthreads();
    flush_pair_add(a.mult + (uint64_t)set * MULT_BINS, s_cnt, half, a.report, s_rep, blockDim.x);
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

__global__ void __launch_bounds__(256) acc_reset_kernel(uint32_t *mult, uint64_t words, uint64_t *report) {
    zero_and_reset(mult, words, report, blockDim.x);
}

}  // namespace aesw_acc

extern "C" {

int aesw_acc_reset_device(aesw_ctx *ctx, uint32_t n_sets, uint32_t *d_mult, aesw_mult_report *d_report, void *stream) {
    using namespace aesw_acc;
    static_assert(sizeof(aesw_mult_report) == 3 * sizeof(uint64_t), "the kernels address the report as three u64");
    const char *const call = "aesw_acc_reset_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_outputs(0, false, n_sets, d_mult, d_report)) return refuse(ctx, call, why);
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
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_layout(layout)) return refuse(ctx, call, why);
    if (const char *why = bad_outputs(k, true, n_sets, d_mult, d_report)) return refuse(ctx, call, why);
    const Placement place(k);
    const uint64_t cap = place.total(n_sets);
    if (first_block > cap || n_blocks > cap - first_block)
        return refuse(ctx, call, "first_block + n_blocks is more than aesw_block_capacity(k, n_sets)", AESW_ERR_CAPACITY);
    if (n_blocks == 0) return AESW_OK;
    if (const char *why = bad_slabs(d_x, d_y, d_z)) return refuse(ctx, call, why);
    RunParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    p.table = ctx->d_chktab[layout == AESW_LAYOUT_DENSE ? 0 : 1];  // uploaded by aesw_create(): nothing is allocated here
    p.tab768 = ctx->d_tables;
    p.mult = d_mult;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    const RunPlan plan = run_plan(place, first_block, n_blocks, blocks_per_workgroup);
    if (!plan.fits()) return refuse(ctx, call, "blocks_per_workgroup leaves more than 2^22 chunks in one set");
    p.run = plan.run;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const dim3 grid((unsigned)(2 * plan.pairs), plan.pieces);
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
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_layout(layout)) return refuse(ctx, call, why);
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
    return aesw::run_default_chunk(n_blocks);
}

}  // extern "C"
