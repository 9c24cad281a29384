// mult/aesw_mult.hip -- libaesw_mult.so (include/aesw_mult.h): the lookup multiplicities of a many-circuit batch, one
// histogram of AESW_TABLE_ROWS bins per (circuit, column set).  (A directory of its own, as it is a library of its own: csrc/
// itself holds the sources of libaesw.so.)  The bin rule and the sizes of the counter split are aesw_mult.h's, the set of a
// block Placement's, and the counting of a staged unit -- row entries, the sinks (and with the LDS one which workgroup of a
// pair owns which bin), block staging, the key slab of a wave, the workgroup's report, the wave count next to the LDS counters
// -- aesw_mult_dev.h's, shared with libaesw_acc.so and libaesw_vacc.so.  What is here is what a workgroup counts and what becomes of its counts, in
// two forms that give the same bytes:
//   * DIRECT: d_mult is zeroed by a launch of its own; workgroups of four waves share a circuit's blocks, and every hit is one
//     global atomic add into the histogram of the block's set;
//   * PRIVATE: two workgroups own one (circuit, set).  Both walk every block of the set, each counts the bins of its half in
//     LDS and stores them once, with plain contiguous stores: no global atomic touches d_mult, and nothing has to zero it
//     first;
// and the entry points: the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's), the choice of
// the form, the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_mult.h"
#include "../aesw_entry.h"
#include "../aesw_mult_dev.h"

namespace aesw_mult {
using namespace aesw;
using namespace aesw::multdev;

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

// The blocks a circuit places: its count clamped to the capacity, whatever the offsets hold.
__device__ __forceinline__ uint64_t placed_blocks(const MultParams &a, uint32_t c, uint64_t &o0) {
    o0 = a.offsets[c];
    const uint64_t o1 = a.offsets[c + 1];
    return o1 > o0 ? (o1 - o0 < a.cap ? o1 - o0 : a.cap) : 0;
}
// Key slab c by one wave, as unit c, ahead of the wave's blocks.
template <int LAYOUT, class Sink>
__device__ __forceinline__ void count_circuit_keys(const MultParams &a, uint32_t c, uint8_t *img, const uint8_t *t768, uint32_t lane, Sink &sink,
                                                   Findings &acc) {
    count_key_slab<LAYOUT>(a, c, img, t768, lane, sink, acc);
    wave_lds_sync();  // a block overwrites the image
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
    Findings acc;
    if (g == 0 && wave == 0 && a.kx) count_circuit_keys<LAYOUT>(a, c, img, t768, lane, sink, acc);  // into set 0
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

// PRIVATE.  grid: two workgroups per (circuit, set)
template <int LAYOUT>
__global__ void __launch_bounds__(CounterGeo<LAYOUT>::WAVES * LANES) mult_private_kernel(const MultParams a) {
    using G = ChkLayout<LAYOUT>;
    constexpr int WAVES = CounterGeo<LAYOUT>::WAVES;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[MULT_COUNTERS];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[WAVES * G::BI];
    __shared__ uint32_t s_t768[768 / 4];
    __shared__ unsigned long long s_rep[3];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    const uint32_t half = blockIdx.x & 1u, unit = blockIdx.x >> 1;
    const uint32_t c = unit / a.n_sets, set = unit - c * a.n_sets;
    const uint8_t *t768 = reinterpret_cast<const uint8_t *>(s_t768);
    uint8_t *img = s_img + wave * G::BI;
    const u32x4 zero = {0, 0, 0, 0};
    for (uint32_t i = threadIdx.x; i < MULT_COUNTERS / 4; i += blockDim.x) reinterpret_cast<u32x4 *>(s_cnt)[i] = zero;
    load_t768(s_t768, a.tab768);
    rep_init(s_rep);
    BlockRows rows;
    rows.load(a.table, lane);
    __syncthreads();
    uint64_t o0;
    const uint64_t n_c = placed_blocks(a, c, o0);
    const uint64_t b0 = o0 + a.place.first_block(set), cnt = a.place.filled(set, n_c);
    LdsSink sink{s_cnt, half};
    Findings acc;
    if (set == 0 && wave == 0 && a.kx) count_circuit_keys<LAYOUT>(a, c, img, t768, lane, sink, acc);
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
    // (the ranges are aesw_mult.h's, taken as constants, half 0's in the order of the bins; nobody counts the zero row)
    constexpr MultFlushRange xr = mult_flush_range(0, 0), xr1 = mult_flush_range(1, 0), lo = mult_flush_range(0, 1), hi = mult_flush_range(0, 2);
    if (half == 0) {
        for (uint32_t i = threadIdx.x; i < lo.length; i += blockDim.x) out[lo.bin + i] = (s_cnt + lo.counter)[i];
        for (uint32_t i = threadIdx.x; i < xr.length; i += blockDim.x) out[xr.bin + i] = (s_cnt + xr.counter)[i];
        for (uint32_t i = threadIdx.x; i < hi.length; i += blockDim.x) out[hi.bin + i] = (s_cnt + lo.counter)[hi.counter - lo.counter + i];
        if (threadIdx.x == 0) out[MULT_ZERO_ROW] = 0;
        rep_flush(a.report, s_rep);
    } else {
        for (uint32_t i = threadIdx.x; i < xr1.length; i += blockDim.x) out[xr1.bin + i] = (s_cnt + xr1.counter)[i];
    }
}

// The report starts as (0 lookups, 0 misses, no miss), and for the DIRECT form d_mult as zeros (zero_and_reset under this
// library's name).  words == 0: the report alone.
__global__ void __launch_bounds__(256) mult_init_kernel(uint32_t *mult, uint64_t words, uint64_t *report) {
    zero_and_reset(mult, words, report, blockDim.x);
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
        if (dense) hipLaunchKernelGGL((mult_private_kernel<DENSE>), grid, dim3(CounterGeo<DENSE>::WAVES * LANES), 0, s, p);
        else hipLaunchKernelGGL((mult_private_kernel<PACKED>), grid, dim3(CounterGeo<PACKED>::WAVES * LANES), 0, s, p);
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

}  // namespace aesw_mult

extern "C" {

int aesw_mult_count_device_form(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, int layout,
                                const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *d_key_slabs, uint32_t *d_mult,
                                aesw_mult_report *d_report, void *stream, int form) {
    using namespace aesw;
    static_assert(sizeof(aesw_mult_report) == 3 * sizeof(uint64_t), "the kernels address the report as three u64");
    constexpr uint32_t MAX_UNITS = 1u << 24;
    const char *const call = "aesw_mult_count_device";  // the public name, whichever of the two was called
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_layout(layout)) return refuse(ctx, call, why);
    if (const char *why = bad_k(k)) return refuse(ctx, call, why);
    if (!mult_sets_ok(n_sets) || n_circuits == 0 || (uint64_t)n_circuits * n_sets > MAX_UNITS)
        return refuse(ctx, call, "n_sets must be 1 ... 1024, n_circuits >= 1 and n_circuits * n_sets <= 2^24");
    if (form != AESW_MULT_FORM_AUTO && form != AESW_MULT_FORM_DIRECT && form != AESW_MULT_FORM_PRIVATE) return refuse(ctx, call, "no such form");
    if (!d_offsets || !aligned_to(d_offsets, 8) || !d_report || !aligned_to(d_report, 8)) return refuse(ctx, call, "d_offsets and d_report must be there and 8-byte aligned");
    if (!d_mult || !aligned_to(d_mult, 16)) return refuse(ctx, call, "d_mult must be there and 16-byte aligned");
    if (const char *why = bad_slabs(d_x, d_y, d_z)) return refuse(ctx, call, why);
    const aesw_key_slab *ks = d_key_slabs;
    if (const char *why = bad_key_columns(ks, k)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    aesw_mult::MultParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    if (with_keys(ks, k)) { p.kx = ks->kx; p.ky = ks->ky; p.kz = ks->kz; }
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
