// vals/aesw_vals_check.hip -- libaesw_vals.so (include/aesw_vals.h): MockProver::assert_satisfied over a VALUES witness in one
// check launch.  (A directory of its own, as it is a library of its own: csrc/ itself holds the sources of libaesw.so.)  The
// checks are aesw_vals_check.h's (a block) and aesw_check.h's (a key slab); the wave's machinery -- the LDS synchronisation, the
// register staging, the branch-free walk of a table, the verdict of a staged key unit, the report flush -- is aesw_check_dev.h's,
// and the launch geometry aesw_internal.h's: the sources check_kernel (libaesw.so) is made of.  What is here is the table and
// the staging:
//   * a block is its 448 y + 608 z + 16 pt (+ 16 ct) bytes, 16-byte loads into registers, issued for the next block before the
//     current one is walked out of LDS; the image is  y | z | pt | key image | ct;
//   * the fast walk takes the 1 056 resolved row entries and no edges (fast_unit_bad<.., NEDGES = 0>); the exact walk
//     (check_values_block) runs only for a block some lane objects to;
//   * a shared key is staged once per wave, in front of its blocks, and checked once, as a unit of its own, by the grid's first
//     wave; with per-block keys the block's key slab travels and is checked with it (key_unit_check).
// Nothing is written but the report (plain C++ stores and atomics), which vals_report_init_kernel resets on the same stream first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../../include/aesw_vals.h"
#include "../aesw_check_dev.h"
#include "../aesw_entry.h"
#include "../aesw_vals_check.h"

namespace aesw_vals {
using namespace aesw;
using KG = ChkLayout<PACKED>;  // the key image's inner offsets and vector widths

constexpr int BI = VALS_BI;                                    // y | z | pt
constexpr int CT_AT = (VALS_BI + VALS_KI + 15) / 16 * 16;      // the block's ciphertext, behind the key image
constexpr int IMG = CT_AT + 16;                                // bytes of one wave's image region: 2 032
static_assert(BI % 16 == 0 && VALS_O_Z % 16 == 0 && VALS_O_PT % 16 == 0, "16-byte units");
static_assert(VALS_KI == KG::KI && (BI + KG::O_KZ) % 8 == 0 && (BI + KG::O_W) % 8 == 0, "the key image is staged with StagedKey<PACKED>");

// The check table (aesw_vals_check.h: device form) of this library, one copy per device, filled by ensure_table().
__device__ uint32_t g_vals_table[CHK_WORDS];

__device__ __forceinline__ void load_vals_fast_table(uint32_t *tab, const uint32_t *t) {
    for (uint32_t r = threadIdx.x; r < (uint32_t)(VALS_ROWS + KEY_ROWS); r += blockDim.x) {
        const uint32_t base = r < (uint32_t)VALS_ROWS ? CHK_ROWS + 2 * r : CHK_KROWS + 2 * (r - VALS_ROWS);
        fast_row_entry(t[base], t[base + 1], tab[base], tab[base + 1]);
    }
    for (uint32_t i = threadIdx.x; i < (uint32_t)(KEY_COPIES + WORDS_ROWS); i += blockDim.x) tab[CHK_KEDGES + i] = t[CHK_KEDGES + i];
}
// tab[VALS_CT_LITERALS + 2 * i]: the low half is the image offset of z of slab row 1344 + i (the last sixteen entries)
constexpr int VALS_CT_LITERALS = CHK_ROWS + 2 * (VALS_ROWS - 16) + 1;

template <bool PBK>
__global__ void __launch_bounds__(256) vals_check_kernel(const CheckParams a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t check_lds[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(check_lds);
    uint8_t *t768 = check_lds + CHK_WORDS * 4;
    const uint32_t wave = threadIdx.x / LANES, lane = threadIdx.x % LANES;
    uint8_t *img = t768 + 768 + wave * IMG;
    uint8_t *kimg = img + BI;
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) reinterpret_cast<uint32_t *>(t768)[i] = reinterpret_cast<const uint32_t *>(a.tab768)[i];
    load_vals_fast_table(tab, a.table);
    __syncthreads();
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / LANES), gwave = (uint64_t)blockIdx.x * (blockDim.x / LANES) + wave;
    CheckAcc acc;
    if (gwave == 0 && lane == 0) { a.report[0] = a.n; a.report[1] = PBK ? a.n : 1; }
    const uint32_t ct_off = tab[VALS_CT_LITERALS + 2 * (lane & 15)] & 0xffffu, w_off = tab[CHK_KEY_LITERALS + (lane & 15)] & 0xffffu;  // lanes 0..15
    if (!PBK) {  // one key slab for the whole batch: every wave keeps a copy behind its block image; the grid's first wave checks it
        StagedKey<PACKED> sk;
        sk.load(a, 0, lane);
        uint32_t klit0 = 0;
        if (lane < 16 && a.keys) klit0 = a.keys[lane];
        sk.store(kimg, lane);
        wave_lds_sync();
        if (gwave == 0) key_unit_check(img, tab, t768, a.table, a.keys, klit0, w_off, 0, lane, acc);
    }
    Staged<Geo<VALUES>::YS, 16> sy; Staged<Geo<VALUES>::ZS, 16> sz;
    StagedKey<PACKED> skey;
    u32x4 lit = {0, 0, 0, 0};  // lane 0: the plaintext, lane 1: the ciphertext
    uint32_t klit = 0;         // lanes 0..15: the key bytes
    auto fetch = [&](uint64_t b) {
        sy.load(a.y + b * Geo<VALUES>::YS, lane); sz.load(a.z + b * Geo<VALUES>::ZS, lane);
        if (PBK) skey.load(a, b, lane);
        if (lane == 0) lit = *reinterpret_cast<const u32x4 *>(a.pt + b * 16);
        if (lane == 1 && a.ct) lit = *reinterpret_cast<const u32x4 *>(a.ct + b * 16);
        if (PBK && lane < 16 && a.keys) klit = a.keys[b * 16 + lane];
    };
    if (gwave < a.n) fetch(gwave);
    for (uint64_t b = gwave; b < a.n; b += nwaves) {
        sy.store(img, lane); sz.store(img + VALS_O_Z, lane);
        if (lane == 0) *reinterpret_cast<u32x4 *>(img + VALS_O_PT) = lit;
        if (lane == 1 && a.ct) *reinterpret_cast<u32x4 *>(img + CT_AT) = lit;
        if (PBK) skey.store(kimg, lane);
        const uint32_t klit_b = klit;
        wave_lds_sync();
        if (b + nwaves < a.n) fetch(b + nwaves);  // in flight while this block is checked
        uint32_t bad = fast_unit_bad<CHK_ROWS, VALS_ROWS, 0, 0>(img, t768, tab, lane);
        if (lane < 16 && a.ct) bad |= img[ct_off] != img[CT_AT + lane];
        if (__ballot(bad != 0) != 0) check_values_block(img, a.table, t768, a.ct ? a.ct + b * 16 : nullptr, b, lane, LANES, acc);
        if (PBK) key_unit_check(img, tab, t768, a.table, a.keys, klit_b, w_off, b, lane, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    flush_acc(a.report, acc);
}

// The report starts as (0 blocks, 0 keys, no failures, first = none): a kernel node, not memset nodes, so a captured graph
// replays it as it runs eagerly.
__global__ void __launch_bounds__(64) vals_report_init_kernel(uint64_t *report) {
    report_reset(report, 7, 1u << 6, threadIdx.x);
}

static hipError_t launch_vals_check(const CheckParams &p, hipStream_t s) {
    hipLaunchKernelGGL(vals_report_init_kernel, dim3(1), dim3(64), 0, s, p.report);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.n == 0) return e;
    const size_t lds = check_lds_bytes(IMG);  // 33 KiB
    const dim3 grid((unsigned)check_groups(p.n)), block(CHECK_WAVES * LANES);
    if (p.per_block_keys) hipLaunchKernelGGL((vals_check_kernel<true>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((vals_check_kernel<false>), grid, block, lds, s, p);
    return hipGetLastError();
}

// The table lives in the code object's own storage: nothing to allocate, nothing to free.  It is filled once per device and
// process; the copy is synchronous, and legal while some stream of this thread is being captured (relaxed capture mode for the
// length of the copy).  Called with the context's device current.
constexpr int MAX_DEVICES = 64;
static int ensure_table(aesw_ctx *ctx, const uint32_t **d_table) {
    static std::mutex mu;
    static const uint32_t *uploaded[MAX_DEVICES] = {};
    if (ctx->device < 0 || ctx->device >= MAX_DEVICES) return AESW_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(mu);
    if (!uploaded[ctx->device]) {
        std::vector<uint32_t> host(CHK_WORDS);
        if (build_values_device_table(host.data()) != 0) {
            ctx->last_error = "aesw_vals: a copy chain of the block does not end in the values image";
            return AESW_ERR_INVALID_ARG;
        }
        void *p = nullptr;
        HIP_TRY(ctx, hipGetSymbolAddress(&p, HIP_SYMBOL(g_vals_table)));
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

}  // namespace aesw_vals

extern "C" {

int aesw_vals_check_device(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n, const uint8_t *d_y,
                           const uint8_t *d_z, const uint8_t *d_ct, const aesw_key_slab *d_key_slab, aesw_check_report *d_report,
                           void *stream) {
    static_assert(sizeof(aesw_check_report) == 7 * sizeof(uint64_t), "the kernel addresses the report as seven u64");
    if (int rc = aesw::entry_refused(ctx, "aesw_vals_check_device")) return rc;
    if (!d_report || !aligned_to(d_report, 8)) return AESW_ERR_INVALID_ARG;
    const aesw_key_slab *ks = d_key_slab;
    if (!key_slab_ok(ks) || !aligned_to(d_keys, 4)) return AESW_ERR_INVALID_ARG;
    if (per_block_keys && n && !d_keys) return AESW_ERR_INVALID_ARG;
    if (n && (!d_pt || !d_y || !d_z || !aligned_to(d_pt, 16) || !aligned_to(d_ct, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16)))
        return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    aesw::CheckParams p{};
    const int rc = aesw_vals::ensure_table(ctx, &p.table);
    if (rc != AESW_OK) return rc;
    p.pt = d_pt; p.keys = d_keys; p.y = d_y; p.z = d_z; p.ct = d_ct;  // x: a values witness has none
    aesw::set_key_slab(p, ks);
    p.tab768 = ctx->d_tables;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.n = n;
    p.per_block_keys = per_block_keys ? 1u : 0u;
    aesw::set_strides(p, aesw::VALS_ST);  // no x; the PACKED key slab
    p.bi = aesw_vals::BI; p.img = aesw_vals::IMG;
    HIP_TRY(ctx, aesw_vals::launch_vals_check(p, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

int aesw_vals_prepare(aesw_ctx *ctx) {
    if (int rc = aesw::entry_refused(ctx, "aesw_vals_prepare")) return rc;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const uint32_t *t = nullptr;
    return aesw_vals::ensure_table(ctx, &t);
}

uint32_t aesw_vals_check_rows(void) { return aesw::VALS_ROWS; }

int aesw_vals_check_table(uint32_t *words, uint16_t *rows) {
    uint32_t w[2 * aesw::VALS_ROWS];
    uint16_t r[aesw::VALS_ROWS];
    if (aesw::build_values_check_table(w, r) != aesw::VALS_ROWS) return AESW_ERR_INVALID_ARG;
    if (words) std::memcpy(words, w, sizeof w);
    if (rows) std::memcpy(rows, r, sizeof r);
    return AESW_OK;
}

uint32_t aesw_vals_image_bytes(void) { return aesw::VALS_BI + aesw::VALS_KI; }

}  // extern "C"
