// aesw_api.cpp -- the C ABI of include/aesw.h on top of the gfx950 kernels: context, geometry, options and the
// device-pointer entry points (the host-pointer ones are aesw_hostpath.cpp).
// Host code only (compiled by hipcc for the HIP runtime API).  There is no CPU
// compute path: without a usable device every computing entry point fails.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/aesw.h"
#include "aesw_internal.h"
#include "aesw_check.h"
#include "aesw_fr.h"

using namespace aesw;

#include "aesw_ctx.h"

namespace {

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool valid_layout(int l) { return aesw_valid_layout(l); }

// The output columns of a key slab (null slab = none wanted); false if one of them is not 16-byte aligned.
bool key_out_of(const aesw_key_slab *ks, KeyOut *ko) {
    *ko = ks ? KeyOut{ks->w, ks->kx, ks->ky, ks->kz} : KeyOut{nullptr, nullptr, nullptr, nullptr};
    return (!ko->w || aligned16(ko->w)) && (!ko->kx || aligned16(ko->kx)) && (!ko->ky || aligned16(ko->ky)) && (!ko->kz || aligned16(ko->kz));
}

uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }

// ---- bn256::Fr Montgomery table: v -> v * 2^256 mod r, 32 B little-endian ----
// r = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
// (halo2curves 0.6.1 bn256::Fr, Cargo.lock:779-781).
// The field is aesw_fr.h's.
void build_fr_lut(uint8_t out[256 * 32]) {
    const FrByteTable t = fr_byte_table();
    std::memcpy(out, t.cell, sizeof t.cell);  // little-endian limbs
}

}  // namespace

static void vmm_release_arena(void *va, size_t total) {
    (void)hipMemUnmap(va, total);
    (void)hipMemAddressFree(va, total);
}

// Waves per group when the option is 0 (auto): as many 16-block waves as keep
// 6-8 waves resident per CU given the LDS windows (DESIGN.md "occupancy").
static int auto_waves(const aesw_ctx *ctx, int layout, bool pbk) {
    // upper bound: a group's staging must stay below 64 KiB (16-bit LDS addresses in the flush descriptors)
    const int max_waves = layout == AESW_LAYOUT_DENSE ? 2 : layout == AESW_LAYOUT_VALUES ? 4 : 3;
    int w;
    // per-block keys: one-wave groups (7 resident per CU instead of two 3-wave groups) measured +1.3 ... +2.4 % at 2^20
    // blocks on two boxes and -0.6 % on a third (tools/sweep.py 20 c2 packed waves); shared key: 3-wave groups
    if (pbk) w = ctx->opt.waves_pbk ? ctx->opt.waves_pbk : 1;
    else w = ctx->opt.waves_shared ? ctx->opt.waves_shared : (layout == AESW_LAYOUT_DENSE ? 2 : 3);
    return w > max_waves ? max_waves : w;
}

// key_kernel alone (tools/keysweep.py, 2^20 keys): packed 4-wave groups, dense 2-wave groups
static int auto_waves_key(const aesw_ctx *ctx, int layout, bool want_rk) {
    // packed, witness only (no round-key output: no 2.8 KB round-key staging per wave since round 4): three 3-wave groups fit a CU
    // (45.7 KB each) and run 143.7 us against 146.3 for 4-wave groups and 148.0 / 154.9 for 2 / 1 (tools/keyarena.py,
    // profiles/r04_study/key_kernel_kz.md); with round keys a 3-wave group is 54 KB (two per CU): 4-wave groups as before
    if (ctx->opt.waves_pbk) return ctx->opt.waves_pbk;
    if (layout == AESW_LAYOUT_DENSE) return 2;
    return want_rk ? 4 : 3;
}

// ---- shared with aesw_hostpath.cpp (declared in aesw_ctx.h) --------------------------------------------------------
int fill_assemble_params(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x, const uint8_t *d_y,
                         const uint8_t *d_z, const aesw_key_slab *ks, AssembleParams *p) {
    if (!ctx || !valid_layout(layout) || layout == AESW_LAYOUT_VALUES /* whole columns need every cell */ || k < 2 || k > 32 ||
        n_sets == 0 || n_sets > 1024)
        return AESW_ERR_INVALID_ARG;
    if (n_blocks && (!d_x || !d_y || !d_z)) return AESW_ERR_INVALID_ARG;
    if (n_blocks > aesw_block_capacity(k, n_sets)) return AESW_ERR_CAPACITY;  // panic in the reference, src/aes128.rs:160-162
    *p = AssembleParams{};
    p->x = d_x; p->y = d_y; p->z = d_z;
    if (ks) { p->kw = ks->w; p->kx = ks->kx; p->ky = ks->ky; p->kz = ks->kz; }
    p->fr_lut = ctx->d_fr_lut;
    p->n_blocks = n_blocks;
    p->k = k;
    p->n_sets = n_sets;
    p->col_first = 0;
    p->col_count = 3 * n_sets + 1;
    set_strides(*p, slab_strides(layout));
    p->packed = layout == AESW_LAYOUT_PACKED;
    p->geometry = ctx->opt.asm_geo;
    return AESW_OK;
}

int check_witness_impl(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n, int layout,
                       const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const uint8_t *d_ct, const aesw_key_slab *ks,
                       aesw_check_report *d_report, void *stream, bool skip_shared_key) {
    static_assert(sizeof(aesw_check_report) == 7 * sizeof(uint64_t), "the kernels address the report as seven u64");
    if (!ctx || !d_report || (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED)) return AESW_ERR_INVALID_ARG;
    if (per_block_keys && n && !d_keys) return AESW_ERR_INVALID_ARG;
    if (n && (!d_pt || !d_x || !d_y || !d_z || !ks || !ks->w || !ks->kx || !ks->ky || !ks->kz)) return AESW_ERR_INVALID_ARG;
    if (n && (!aligned4(d_pt) || !aligned4(d_x) || !aligned4(d_y) || !aligned4(d_z) || !aligned4(ks->w) || !aligned4(ks->kx) || !aligned4(ks->ky) ||
              !aligned4(ks->kz) || (reinterpret_cast<uintptr_t>(d_report) & 7u)))
        return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const int li = layout == AESW_LAYOUT_DENSE ? 0 : 1;  // the check tables were uploaded by aesw_create(): nothing is allocated here
    const CheckGeo cg = check_geo(layout);
    CheckParams p{};
    p.pt = d_pt; p.keys = d_keys; p.x = d_x; p.y = d_y; p.z = d_z; p.ct = d_ct;
    if (ks) set_key_slab(p, ks);
    p.table = ctx->d_chktab[li];
    p.tab768 = ctx->d_tables;
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.n = n;
    p.per_block_keys = per_block_keys ? 1u : 0u;
    p.skip_shared_key = skip_shared_key ? 1u : 0u;
    set_strides(p, slab_strides(layout));  // DENSE or PACKED (checked above): check_geo's domain
    p.bi = cg.bi;
    p.img = (cg.bi + cg.ki + 15u) & ~15u;
    HIP_TRY(ctx, launch_check(p, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

// ---- one encrypt launch, and the internal streams several of them are dealt onto ----------------------------------
namespace {

// One aesw_encrypt_witness_device call whose arguments have passed validate_encrypt
struct EncLaunch {
    const uint8_t *d_pt, *d_keys;
    int per_block_keys;
    uint64_t n;
    int layout;
    uint8_t *d_x, *d_y, *d_z, *d_ct;
    KeyOut ko;
    bool kemit;  // a key slab is wanted
};

// The argument checks of aesw_encrypt_witness_device, statuses in this order.  True: *L is a launch to issue.  False: there is none,
// and *status is what the call returns (an error, or AESW_OK for n == 0).
bool validate_encrypt(const aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n, int layout, uint8_t *d_x,
                     uint8_t *d_y, uint8_t *d_z, uint8_t *d_ct, const aesw_key_slab *ks, EncLaunch *L, int *status) {
    *status = AESW_ERR_INVALID_ARG;
    if (!ctx || !valid_layout(layout)) return false;
    if (!d_keys) {
        if (per_block_keys) return false;
        if (!ctx->keys.has_key()) { *status = AESW_ERR_NO_KEY; return false; }  // "Keys should be scheduled", src/aes128.rs:170
    }
    *L = EncLaunch{d_pt, d_keys, per_block_keys, n, layout, d_x, d_y, d_z, d_ct, KeyOut{nullptr, nullptr, nullptr, nullptr}, false};
    *status = AESW_OK;
    if (n == 0) return false;
    *status = AESW_ERR_INVALID_ARG;
    const bool has_x = slab_strides(layout).x != 0;  // AESW_LAYOUT_VALUES has no x column: d_x is ignored
    if (!d_pt || (has_x && !d_x) || !d_y || !d_z) return false;
    if ((has_x && !aligned16(d_x)) || !aligned16(d_y) || !aligned16(d_z) || !aligned4(d_pt) || (d_keys && !aligned4(d_keys)) ||
        (d_ct && !aligned4(d_ct)))
        return false;
    if (!key_out_of(ks, &L->ko)) return false;
    L->kemit = L->ko.w || L->ko.kx || L->ko.ky || L->ko.kz;
    if (!d_keys && L->kemit) return false;  // the key slab of a scheduled key comes from aesw_schedule_key*
    *status = AESW_OK;
    return true;
}

// One validated launch (n > 0) on one stream: the shared key's slab, the order behind a scheduled key, the kernel, the reader's mark.
// The caller holds the DeviceGuard.
int enqueue_encrypt(aesw_ctx *ctx, const EncLaunch &L, hipStream_t s) {
    if (!L.per_block_keys && L.kemit) {
        // shared key: its schedule witness is one key slab
        KeyParams kp{L.d_keys, ctx->d_tables, L.ko, nullptr, 1, 0, 0};
        HIP_TRY(ctx, launch_key(kp, L.layout, ctx->xt, 1, ctx->opt.key_nt, 0u, s));
    }
    const int km = L.per_block_keys ? 0 : (L.d_keys ? 1 : 2);
    KeyRing::Access rd;
    if (km == 2) {  // capture status is asked for scheduled-key launches only: the other key modes make no runtime call but the launch
        const int rc = ctx->keys.begin_read(ctx, s, &rd);
        if (rc != AESW_OK) return rc;
    }
    EncParams p{L.d_pt, L.d_keys, reinterpret_cast<const uint32_t *>(rd.d), ctx->d_tables, ctx->d_ftab[L.layout], L.d_x, L.d_y, L.d_z, L.d_ct,
                L.per_block_keys ? L.ko : KeyOut{nullptr, nullptr, nullptr, nullptr}, L.n, 0, 0};
#ifdef AESW_TRACE
    p.trace = ctx->trace;
#endif
    HIP_TRY(ctx, launch_encrypt(p, L.layout, ctx->xt, km, L.per_block_keys && L.kemit, auto_waves(ctx, L.layout, L.per_block_keys != 0),
                                ctx->opt.nt, (uint32_t)ctx->opt.grid_cap, ctx->opt.xcd_remap, (uint32_t)ctx->opt.lds_pad, s));
    return km == 2 ? ctx->keys.end_read(ctx, rd) : AESW_OK;  // this launch reads the current slot: nothing may overwrite the slot under it
}

// Fork / join of the internal streams: `ns` of them (at most 8, made on first use) start behind what `s` holds, issue(i, stream)
// puts item i of `count` on internal stream i mod ns until one fails, and `s` continues behind all of them -- also after a failure:
// what was issued must be ordered before whatever the caller does next on `s`.
template <class Issue>
int fork_join(aesw_ctx *ctx, hipStream_t s, uint32_t ns, uint32_t count, Issue &&issue) {
    if (!ctx->ev_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (uint32_t j = 0; j < ns; ++j) {
        if (!ctx->s_batch[j]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_batch[j], hipStreamNonBlocking));
        if (!ctx->ev_join[j]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join[j], hipEventDisableTiming));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
    for (uint32_t j = 0; j < ns; ++j) HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_batch[j], ctx->ev_fork, 0));
    int rc = AESW_OK;
    for (uint32_t i = 0; i < count && rc == AESW_OK; ++i) rc = issue(i, ctx->s_batch[i % ns]);
    for (uint32_t j = 0; j < ns; ++j) {
        const hipError_t e1 = hipEventRecord(ctx->ev_join[j], ctx->s_batch[j]);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(s, ctx->ev_join[j], 0) : e1;
        if (e2 != hipSuccess && rc == AESW_OK) rc = fail_hip(ctx, e2, "join of the batch streams");
    }
    return rc;
}

// A LONE launch on the caller's stream: aesw_encrypt_witness_device (the chunks of the host-pointer paths come through it), and the
// batches of the batch entry point when it has one stream or one batch.  Only here does "split_small" apply.
int encrypt_lone(aesw_ctx *ctx, const EncLaunch &L, hipStream_t s) {
    if (ctx->opt.split_small <= 1 || L.per_block_keys || L.kemit || L.n < ((uint64_t)1 << 15) || L.n > ((uint64_t)1 << 17)) return enqueue_encrypt(ctx, L, s);
    // "split_small": the lone small batch as 2-3 sub-launches on the internal streams.  Sub-ranges are multiples of 48 blocks -- whole
    // 3-wave groups, and 48 x 1360 / 1056 / 608 are multiples of the 128-byte line, so no two sub-launches share a line of any column.
    // A split uses as many internal streams as it has parts (at most 8, at least 2 for these n), whatever "batch_streams" says.
    const uint32_t parts = (uint32_t)ctx->opt.split_small;
    const uint64_t per = ((L.n + parts - 1) / parts + 47) / 48 * 48;
    const uint32_t cnt = (uint32_t)((L.n + per - 1) / per);
    const SlabStrides st = slab_strides(L.layout);
    return fork_join(ctx, s, cnt, cnt, [&](uint32_t i, hipStream_t si) {
        const uint64_t lo = i * per;
        EncLaunch part = L;
        part.d_pt += lo * 16;
        part.n = L.n - lo < per ? L.n - lo : per;
        if (L.d_x) part.d_x += lo * st.x;
        part.d_y += lo * st.y;
        part.d_z += lo * st.z;
        if (L.d_ct) part.d_ct += lo * 16;
        return enqueue_encrypt(ctx, part, si);
    });
}

}  // namespace

extern "C" {

int aesw_version(void) { return AESW_VERSION; }

const char *aesw_strerror(int status) {
    switch (status) {
    case AESW_OK: return "ok";
    case AESW_ERR_INVALID_ARG: return "invalid argument";
    case AESW_ERR_NO_DEVICE: return "no usable gfx950 device (this library has no CPU path)";
    case AESW_ERR_HIP: return "HIP runtime error";
    case AESW_ERR_NOMEM: return "out of memory";
    case AESW_ERR_CAPACITY: return "AES calls too many. doesn't fit in the rows";
    case AESW_ERR_NO_KEY: return "Keys should be scheduled";
    case AESW_ERR_MISMATCH: return "host value disagrees with the device witness";
    case AESW_ERR_UNSATISFIED: return "constraint system not satisfied";
    case AESW_ERR_COMM: return "RCCL unavailable or a collective call failed";
    default: return "unknown status";
    }
}

const char *aesw_last_error(const aesw_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int aesw_device_count(int *count) {
    if (!count) return AESW_ERR_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n > 0 ? AESW_OK : AESW_ERR_NO_DEVICE;
}

int aesw_create(aesw_ctx **out, int device, const uint8_t sbox[256], const uint8_t mul2[256],
                const uint8_t mul3[256]) {
    if (!out || !sbox || !mul2 || !mul3) return AESW_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AESW_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return AESW_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return AESW_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return AESW_ERR_NO_DEVICE;  // code objects are gfx950 only
    aesw_ctx *ctx = new (std::nothrow) aesw_ctx;
    if (!ctx) return AESW_ERR_NOMEM;
    ctx->device = device;
    DeviceGuard g(device);
    if (!g.ok) { delete ctx; return AESW_ERR_NO_DEVICE; }
    uint8_t host[768];
    std::memcpy(host, sbox, 256);
    std::memcpy(host + 256, mul2, 256);
    std::memcpy(host + 512, mul3, 256);
    ctx->xt = true;
    for (int i = 0; i < 256; ++i)
        if (mul2[i] != xtime((uint8_t)i) || mul3[i] != (uint8_t)(xtime((uint8_t)i) ^ i)) ctx->xt = false;
    uint8_t lut[256 * 32];
    build_fr_lut(lut);
    int rc = AESW_OK;
    auto T = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == AESW_OK) rc = fail_hip(ctx, e, what);
    };
    T(hipMalloc(reinterpret_cast<void **>(&ctx->d_tables), 768), "hipMalloc(tables)");
    T(hipMalloc(reinterpret_cast<void **>(&ctx->d_fr_lut), sizeof lut), "hipMalloc(fr_lut)");
    // the flush schedules depend on the layout only: searched once per process (~20 ms each), uploaded per context
    static std::vector<uint32_t> host_ftab[3];
    static std::once_flag ftab_once;
    std::call_once(ftab_once, [] {
        for (int l = 0; l < 3; ++l) {
            host_ftab[l].resize((size_t)flush_table_words(l));
            build_flush_tables(l, host_ftab[l].data());
        }
    });
    for (int l = 0; l < 3 && rc == AESW_OK; ++l) {
        const std::vector<uint32_t> &ft = host_ftab[l];
        T(hipMalloc(reinterpret_cast<void **>(&ctx->d_ftab[l]), ft.size() * sizeof(uint32_t)), "hipMalloc(flush table)");
        if (rc == AESW_OK) T(hipMemcpy(ctx->d_ftab[l], ft.data(), ft.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(flush table)");
    }
    for (int li = 0; li < 2 && rc == AESW_OK; ++li) {  // check tables of the DENSE / PACKED layout (aesw_check.h): 24 KiB each
        std::vector<uint32_t> ct((size_t)CHK_WORDS);
        build_check_table(li == 0 ? AESW_LAYOUT_DENSE : AESW_LAYOUT_PACKED, ct.data());
        T(hipMalloc(reinterpret_cast<void **>(&ctx->d_chktab[li]), ct.size() * sizeof(uint32_t)), "hipMalloc(check table)");
        if (rc == AESW_OK) T(hipMemcpy(ctx->d_chktab[li], ct.data(), ct.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(check table)");
    }
    if (rc == AESW_OK) rc = ctx->keys.init(ctx);  // the first chunk of round-key slots
    if (rc == AESW_OK) T(warm_launch_attributes(), "hipFuncSetAttribute(max dynamic LDS)");
    if (rc == AESW_OK) T(hipMemcpy(ctx->d_tables, host, 768, hipMemcpyHostToDevice), "hipMemcpy(tables)");
    if (rc == AESW_OK) T(hipMemcpy(ctx->d_fr_lut, lut, sizeof lut, hipMemcpyHostToDevice), "hipMemcpy(fr_lut)");
    if (rc != AESW_OK) {
        aesw_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return AESW_OK;
}

void aesw_destroy(aesw_ctx *ctx) {
    if (!ctx) return;
    if (aesw_is_group(ctx)) return aesw_group_destroy(ctx);
    {
        DeviceGuard g(ctx->device);
        // nothing below may unmap, free or recycle what a launch still queued on any stream uses
        (void)hipDeviceSynchronize();
        if (ctx->s_compute) (void)hipStreamDestroy(ctx->s_compute);
        if (ctx->s_copy) (void)hipStreamDestroy(ctx->s_copy);
        for (int j = 0; j < 8; ++j) {
            if (ctx->s_batch[j]) (void)hipStreamDestroy(ctx->s_batch[j]);
            if (ctx->ev_join[j]) (void)hipEventDestroy(ctx->ev_join[j]);
        }
        if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
        for (int i = 0; i < 2; ++i)
            if (ctx->bounce[i]) (void)hipHostFree(ctx->bounce[i]);
        if (ctx->scratch) (void)hipFree(ctx->scratch);
        for (auto &a : ctx->vmm_arenas)
            for (auto &r : a.ranges) { if (r.vmm) vmm_release_arena(r.p, r.bytes); else (void)hipFree(r.p); }
        aesw_arena_cache_trim(ctx, 0);
        if (ctx->d_tables) (void)hipFree(ctx->d_tables);
        if (ctx->d_fr_lut) (void)hipFree(ctx->d_fr_lut);
        ctx->keys.destroy();
        for (uint32_t *t : ctx->d_ftab)
            if (t) (void)hipFree(t);
        for (uint32_t *t : ctx->d_chktab)
            if (t) (void)hipFree(t);
    }
    delete ctx;
}

int aesw_device(const aesw_ctx *ctx) { return ctx ? ctx->device : -1; }
int aesw_uses_xtime_path(const aesw_ctx *ctx) {
    if (aesw_is_group(ctx)) return aesw_uses_xtime_path(ctx->members[0]);
    return ctx && ctx->xt ? 1 : 0;
}

// ---- geometry ------------------------------------------------------------------

// columns x, y, z and kx, ky, kz of slab_strides(layout), which is all zero for a layout that is none
uint32_t aesw_column_stride(int layout, int col) { return col < 0 || col > 2 ? 0 : slab_strides(layout)[col]; }
uint32_t aesw_key_column_stride(int layout, int col) { return col < 0 || col > 2 ? 0 : slab_strides(layout)[4 + col]; }

int aesw_packed_index(int col, int32_t idx[AESW_AES_ROWS]) {
    if (col < 0 || col > 2 || !idx) return AESW_ERR_INVALID_ARG;
    uint8_t mask[AES_ROWS];
    encrypt_assigned_mask(col, mask);
    mask_to_index(mask, AES_ROWS, idx);
    return AESW_OK;
}

int aesw_layout_index(int layout, int col, int32_t idx[AESW_AES_ROWS]) {
    if (!valid_layout(layout) || col < 0 || col > 2 || !idx) return AESW_ERR_INVALID_ARG;
    if (layout == AESW_LAYOUT_DENSE) {
        for (int r = 0; r < AES_ROWS; ++r) idx[r] = r;
        return AESW_OK;
    }
    if (layout == AESW_LAYOUT_PACKED) return aesw_packed_index(col, idx);
    uint8_t mask[AES_ROWS];
    encrypt_values_mask(col, mask);
    mask_to_index(mask, AES_ROWS, idx);
    return AESW_OK;
}

int aesw_key_packed_index(int col, int32_t idx[AESW_KEY_ROWS]) {
    if (col < 0 || col > 2 || !idx) return AESW_ERR_INVALID_ARG;
    uint8_t mask[KEY_ROWS];
    key_assigned_mask(col, mask);
    mask_to_index(mask, KEY_ROWS, idx);
    return AESW_OK;
}

static_assert(sizeof(aesw_copy_edge) == sizeof(CopyEdge) && sizeof(CopyEdge) == 8, "copy edge layout");
int aesw_block_copy_graph(aesw_copy_edge edges[AESW_BLOCK_COPIES]) {
    if (!edges) return AESW_ERR_INVALID_ARG;
    static_assert(AESW_BLOCK_COPIES == BLOCK_COPIES, "block copies");
    return block_copy_graph(reinterpret_cast<CopyEdge *>(edges)) == BLOCK_COPIES ? AESW_OK : AESW_ERR_INVALID_ARG;
}
int aesw_key_copy_graph(aesw_copy_edge edges[AESW_KEY_COPIES]) {
    if (!edges) return AESW_ERR_INVALID_ARG;
    static_assert(AESW_KEY_COPIES == KEY_COPIES, "key copies");
    return key_copy_graph(reinterpret_cast<CopyEdge *>(edges)) == KEY_COPIES ? AESW_OK : AESW_ERR_INVALID_ARG;
}

int aesw_selector_tags(uint8_t enc_tag[AESW_AES_ROWS], uint8_t key_tag[AESW_KEY_ROWS], uint8_t q_eq_rcon[AESW_WORDS_ROWS],
                       uint8_t rcon_fixed[AESW_WORDS_ROWS]) {
    uint8_t e[AES_ROWS], k[KEY_ROWS], q[WORDS_ROWS], c[WORDS_ROWS];
    encrypt_selector_tags(e);
    key_selector_tags(k, q, c);
    if (enc_tag) std::memcpy(enc_tag, e, sizeof e);
    if (key_tag) std::memcpy(key_tag, k, sizeof k);
    if (q_eq_rcon) std::memcpy(q_eq_rcon, q, sizeof q);
    if (rcon_fixed) std::memcpy(rcon_fixed, c, sizeof c);
    return AESW_OK;
}

// The placement rule of FixedAes128Config::aes_callable (src/aes128.rs:303-325) is aesw_placement.h's.
uint64_t aesw_block_capacity(uint32_t k, uint32_t n_sets) {
    if (k > 40 || n_sets == 0) return 0;
    return Placement(k).total(n_sets);
}

int aesw_block_placement(uint32_t k, uint32_t n_sets, uint64_t b, uint32_t *set, uint64_t *row) {
    if (k > 40 || n_sets == 0 || !set || !row) return AESW_ERR_INVALID_ARG;
    const Placement pl(k);
    if (b >= pl.total(n_sets)) return AESW_ERR_CAPACITY;
    uint64_t bi;
    pl.locate(b, *set, bi);
    *row = Placement::row_of(*set, bi);
    return AESW_OK;
}

int aesw_assemble_selectors(uint32_t k, uint32_t n_sets, uint64_t n_blocks, uint8_t *selectors, uint8_t *fixed) {
    if (k < 2 || k > 32 || n_sets == 0 || n_sets > 1024 || !selectors) return AESW_ERR_INVALID_ARG;
    if (n_blocks > aesw_block_capacity(k, n_sets)) return AESW_ERR_CAPACITY;
    const uint64_t rows = (uint64_t)1 << k;
    uint8_t enc[AES_ROWS], key[KEY_ROWS], q[WORDS_ROWS], rc[WORDS_ROWS];
    encrypt_selector_tags(enc);
    key_selector_tags(key, q, rc);
    std::memset(selectors, 0, (size_t)(5 * n_sets + 1) * rows);
    if (fixed) std::memset(fixed, 0, rows);
    auto sel = [&](uint32_t set, int tag) { return selectors + (size_t)(5 * set + (tag - 1)) * rows; };  // tag 1..5 = selector order
    if (rows >= KEY_ROWS)
        for (uint32_t r = 0; r < KEY_ROWS; ++r)
            if (key[r]) sel(0, key[r])[r] = 1;
    for (uint32_t r = 0; r < WORDS_ROWS && r < rows; ++r) {
        selectors[(size_t)(5 * n_sets) * rows + r] = q[r];
        if (fixed) fixed[r] = rc[r];
    }
    const Placement pl(k);
    for (uint64_t b = 0; b < n_blocks; ++b) {  // below the capacity: checked above
        uint32_t set;
        uint64_t bi;
        pl.locate(b, set, bi);
        const uint64_t row = Placement::row_of(set, bi);
        for (uint32_t r = 0; r < AES_ROWS; ++r)
            if (enc[r]) sel(set, enc[r])[row + r] = 1;
    }
    return AESW_OK;
}

// ---- options --------------------------------------------------------------------

// One row of AESW_OPTIONS (aesw_options.h) per name checks the value and stores it in ctx->opt; here is what a row cannot say.
int aesw_set_option(aesw_ctx *ctx, const char *name, int64_t value) {
    if (aesw_is_group(ctx)) return aesw_group_set_option(ctx, name, value);
    if (!ctx || !name) return AESW_ERR_INVALID_ARG;
    const OptionRow *r = aesw_find_option(name);
    if (!r || !aesw_option_set(ctx->opt, *r, value)) return AESW_ERR_INVALID_ARG;
    switch (r->extra) {
    case OptExtra::ARENA_CACHE: if (!value) aesw_arena_cache_trim(ctx, 0); break;
    case OptExtra::ARENA_CACHE_MAX_MB: aesw_arena_cache_trim(ctx, ctx->opt.arena_cache_max_bytes()); break;
    case OptExtra::KEY_SLOTS: ctx->keys.set_ring_size((int)value); break;
    case OptExtra::FORCE_TABLE_PATH: if (value) ctx->xt = false; break;
#ifdef AESW_TRACE
    case OptExtra::TRACE_PTR: ctx->trace = reinterpret_cast<uint64_t *>(value); break;
#endif
    default: break;
    }
    return AESW_OK;
}

int aesw_get_option(const aesw_ctx *ctx, const char *name, int64_t *value) {
    if (aesw_is_group(ctx)) return aesw_get_option(ctx->members[0], name, value);  // a group: member 0
    if (!ctx || !name || !value) return AESW_ERR_INVALID_ARG;
    const OptionRow *r = aesw_find_option(name);
    if (!r || !(r->access & OPT_GET)) return AESW_ERR_INVALID_ARG;
    if (aesw_option_get(ctx->opt, *r, value)) return AESW_OK;
    switch (r->extra) {
    case OptExtra::KEY_SLOTS: *value = ctx->keys.ring_size(); break;
    case OptExtra::FORCE_TABLE_PATH: *value = ctx->xt ? 0 : 1; break;
    case OptExtra::EFFECTIVE_WAVES_SHARED: *value = auto_waves(ctx, AESW_LAYOUT_PACKED, false); break;
    case OptExtra::EFFECTIVE_WAVES_PBK: *value = auto_waves(ctx, AESW_LAYOUT_PACKED, true); break;
    case OptExtra::EFFECTIVE_WAVES_KEY: *value = auto_waves_key(ctx, AESW_LAYOUT_PACKED, false); break;
    case OptExtra::EFFECTIVE_COPY_THREADS: *value = auto_copy_threads(ctx); break;
    case OptExtra::ARENA_CACHE_HITS: *value = (int64_t)ctx->arena_cache_hits; break;
    case OptExtra::ARENA_CACHED_BYTES: *value = 0; for (const auto &c : ctx->arena_cache) *value += (int64_t)c.cols.bytes; break;
    case OptExtra::KEY_READER_WAITS: *value = (int64_t)ctx->keys.key_reader_waits(); break;
    case OptExtra::KEY_WRITER_WAITS: *value = (int64_t)ctx->keys.key_writer_waits(); break;
    case OptExtra::KEY_SLOTS_ALLOCATED: *value = ctx->keys.key_slots_allocated(); break;
    case OptExtra::KEY_SLOTS_PINNED: *value = ctx->keys.key_slots_pinned(); break;
    // no default: -Wswitch names an OptExtra that has no case here (a readable row has a field or a case above)
    case OptExtra::NONE: case OptExtra::ARENA_CACHE: case OptExtra::ARENA_CACHE_MAX_MB: case OptExtra::TRACE_PTR: return AESW_ERR_INVALID_ARG;
    }
    return AESW_OK;
}

// ---- device-pointer entry points ------------------------------------------------

int aesw_schedule_key_device(aesw_ctx *ctx, const uint8_t *d_key, int layout, const aesw_key_slab *ks, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_schedule_key_device");
    if (!ctx || !valid_layout(layout) || !d_key || !aligned4(d_key)) return AESW_ERR_INVALID_ARG;
    KeyOut ko;
    if (!key_out_of(ks, &ko)) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    KeyRing::Access w;
    const int rc = ctx->keys.begin_write(ctx, s, &w);
    if (rc != AESW_OK) return rc;
    KeyParams kp{d_key, ctx->d_tables, ko, w.d, 1, 0, 0};
    return ctx->keys.end_write(ctx, w, launch_key(kp, layout, ctx->xt, 1, ctx->opt.key_nt, 0u, s));
}

int aesw_encrypt_witness_device(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys,
                                uint64_t n, int layout, uint8_t *d_x, uint8_t *d_y, uint8_t *d_z, uint8_t *d_ct,
                                const aesw_key_slab *ks, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_encrypt_witness_device");
    EncLaunch L;
    int rc;
    if (!validate_encrypt(ctx, d_pt, d_keys, per_block_keys, n, layout, d_x, d_y, d_z, d_ct, ks, &L, &rc)) return rc;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    return encrypt_lone(ctx, L, reinterpret_cast<hipStream_t>(stream));
}

int aesw_encrypt_witness_batches_device(aesw_ctx *ctx, const aesw_batch *batches, uint32_t count, int per_block_keys, int layout,
                                        void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_encrypt_witness_batches_device");
    if (!ctx || !valid_layout(layout) || (count && !batches)) return AESW_ERR_INVALID_ARG;
    if (count == 0) return AESW_OK;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // a batch is checked when its turn comes: the batches in front of a refused one have been issued (and are joined)
    auto issue = [&](uint32_t i, hipStream_t si, bool lone) {
        const aesw_batch &b = batches[i];
        EncLaunch L;
        int rc;
        if (!validate_encrypt(ctx, b.d_pt, b.d_keys, per_block_keys, b.n, layout, b.d_x, b.d_y, b.d_z, b.d_ct, b.d_key_slab, &L, &rc)) return rc;
        return lone ? encrypt_lone(ctx, L, si) : enqueue_encrypt(ctx, L, si);
    };
    const uint32_t ns = (uint32_t)ctx->opt.batch_streams < count ? (uint32_t)ctx->opt.batch_streams : count;
    if (ns <= 1) {  // nothing to overlap: plain launches on the caller's stream, each of them a lone launch ("split_small" applies)
        for (uint32_t i = 0; i < count; ++i) {
            const int rc = issue(i, s, true);
            if (rc != AESW_OK) return rc;
        }
        return AESW_OK;
    }
    // batches dealt onto the internal streams are never split again
    return fork_join(ctx, s, ns, count, [&](uint32_t i, hipStream_t si) { return issue(i, si, false); });
}

int aesw_key_schedule_witness_device(aesw_ctx *ctx, const uint8_t *d_keys, uint64_t n, int layout, uint8_t *d_w,
                                     uint8_t *d_kx, uint8_t *d_ky, uint8_t *d_kz, uint8_t *d_rk, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_key_schedule_witness_device");
    if (!ctx || !valid_layout(layout)) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!d_keys || !aligned4(d_keys)) return AESW_ERR_INVALID_ARG;
    const aesw_key_slab slab{d_w, d_kx, d_ky, d_kz};
    KeyOut ko;
    if (!key_out_of(&slab, &ko) || (d_rk && !aligned16(d_rk))) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    KeyParams kp{d_keys, ctx->d_tables, ko, d_rk, n, 0, 0};
    HIP_TRY(ctx, launch_key(kp, layout, ctx->xt, auto_waves_key(ctx, layout, d_rk != nullptr), ctx->opt.key_nt, ctx->opt.xcd_remap, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

int aesw_lookup_table_device(aesw_ctx *ctx, uint8_t *d_t0, uint8_t *d_t1, uint8_t *d_t2, uint8_t *d_t3, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_lookup_table_device");
    if (!ctx || !d_t0 || !d_t1 || !d_t2 || !d_t3) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    HIP_TRY(ctx, launch_table(ctx->d_tables, d_t0, d_t1, d_t2, d_t3, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

int aesw_assemble_advice_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x,
                                const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *ks, int as_fr, uint8_t *d_out,
                                void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_assemble_advice_device");
    if (!d_out || !aligned16(d_out)) return AESW_ERR_INVALID_ARG;
    AssembleParams p;
    const int rc = fill_assemble_params(ctx, k, n_sets, n_blocks, layout, d_x, d_y, d_z, ks, &p);
    if (rc != AESW_OK) return rc;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    p.out = d_out;
    HIP_TRY(ctx, launch_assemble(p, as_fr != 0, ctx->opt.fr_nt, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

int aesw_check_witness_device(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n, int layout,
                              const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const uint8_t *d_ct, const aesw_key_slab *ks,
                              aesw_check_report *d_report, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_check_witness_device");
    return check_witness_impl(ctx, d_pt, d_keys, per_block_keys, n, layout, d_x, d_y, d_z, d_ct, ks, d_report, stream, false);
}

int aesw_expand_fr_device(aesw_ctx *ctx, const uint8_t *d_cells, uint64_t n_cells, uint8_t *d_fr, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_expand_fr_device");
    if (!ctx) return AESW_ERR_INVALID_ARG;
    if (n_cells == 0) return AESW_OK;
    if (!d_cells || !d_fr || !aligned16(d_fr)) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    HIP_TRY(ctx, launch_expand_fr(d_cells, n_cells, ctx->d_fr_lut, d_fr, ctx->opt.fr_nt, ctx->opt.fr_geo, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

}  // extern "C"
