// circ/aesw_circ_check.hip -- libaesw_circ.so (include/aesw_circ.h): MockProver::assert_satisfied over a many-circuit batch in
// one launch.  (A directory of its own, as it is a library of its own: csrc/ itself holds the sources of libaesw.so.)  The checks are aesw_check.h's; the wave's machinery, the verdict of a staged
// unit, the offset validation and the report flush are aesw_check_dev.h's, and the launch geometry aesw_internal.h's -- the
// sources check_kernel (libaesw.so) is made of.  What is here is the staging, shaped on check_kernel's per-block-key form: four-wave workgroups, one unit per wave at a time,
// the next block's loads issued into registers before the current one is checked out of LDS, a branch-free fast path, and the
// exact second walk (check_block / check_key) only for a unit some lane objects to.  What differs:
//   * block b is held against key slab circuit(b) (aesw_circ_search.h: a wave-uniform binary search over the offsets, scalar
//     loads), fetched with the block: a wave's consecutive blocks are gridDim * 4 apart, so the circuit changes nearly every step;
//   * the C key slabs are units of their own, strided over the grid's waves like the blocks: a key slab is walked once, not
//     once per block, and its 936 B come from HBM once however many blocks copy from it;
//   * the offsets are validated by the lanes of the grid, one circuit per lane, and counted in the report's eighth word.
// Nothing is written but the report (plain C++ stores and atomics), which circ_report_init_kernel resets on the same stream first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_circ.h"
#include "../aesw_check_dev.h"
#include "../aesw_circ_search.h"
#include "../aesw_entry.h"

namespace aesw_circ {
using namespace aesw;

struct CircCheckParams {
    CheckParams c;            // pt, keys (C x 16 or null), x / y / z, ct, the C key slabs, tables, report (8 x u64), n
    const uint64_t *offsets;  // C + 1 (device)
    uint64_t cap;             // aesw_block_capacity(k, n_sets)
    uint32_t n_circuits;
};

template <int LAYOUT>
__global__ void __launch_bounds__(256) circ_check_kernel(const CircCheckParams p) {
    using G = ChkLayout<LAYOUT>;
    const CheckParams &a = p.c;
    extern __shared__ __attribute__((aligned(16))) uint8_t check_lds[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(check_lds);
    uint8_t *t768 = check_lds + CHK_WORDS * 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;  // wave: an SGPR, so is circuit(b)
    uint8_t *img = t768 + 768 + wave * G::IMG;
    uint8_t *kimg = img + G::BI;
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) reinterpret_cast<uint32_t *>(t768)[i] = reinterpret_cast<const uint32_t *>(a.tab768)[i];
    load_fast_table(tab, a.table);
    __syncthreads();
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / LANES), gwave = (uint64_t)blockIdx.x * (blockDim.x / LANES) + wave;
    const uint64_t nc = p.n_circuits;
    CheckAcc acc;
    if (gwave == 0 && lane == 0) { a.report[0] = a.n; a.report[1] = nc; }
    const uint32_t ct_off = tab[CHK_CT_LITERALS + 2 * (lane & 15)] & 0xffffu, w_off = tab[CHK_KEY_LITERALS + (lane & 15)] & 0xffffu;  // lanes 0..15
    const uint32_t off_bad = offsets_bad(p.offsets, nc, a.n, p.cap, gwave, nwaves, lane);

    // the key slabs: unit c, also for a circuit that holds no block
    for (uint64_t c = gwave; c < nc; c += nwaves) {
        StagedKey<LAYOUT> sk;
        sk.load(a, c, lane);
        uint32_t klit = 0;
        if (lane < 16 && a.keys) klit = a.keys[c * 16 + lane];
        sk.store(kimg, lane);
        wave_lds_sync();
        key_unit_check(img, tab, t768, a.table, a.keys, klit, w_off, c, lane, acc);
        wave_lds_sync();  // the next unit overwrites the key image
    }

    // the blocks: every index below n, every key slab index in [0, C)
    Staged<G::SX, 16> sx; Staged<G::SY, 16> sy; Staged<G::SZ, 16> sz;
    StagedKey<LAYOUT> skey;
    uint32_t lit = 0;  // the literal rows: plaintext, ciphertext (lanes 0..15, one byte each)
    typedef const uint64_t __attribute__((address_space(4))) *ConstOffsets;  // read-only for the whole launch: scalar loads
    const ConstOffsets offs = (ConstOffsets)p.offsets;
    auto fetch = [&](uint64_t b) {
        const uint32_t c = circuit_of_block(offs, p.n_circuits, uni64(b));
        sx.load(a.x + b * G::SX, lane); sy.load(a.y + b * G::SY, lane); sz.load(a.z + b * G::SZ, lane);
        skey.load(a, c, lane);
        if (lane < 16) {
            lit = a.pt[b * 16 + lane];
            if (a.ct) lit |= (uint32_t)a.ct[b * 16 + lane] << 8;
        }
    };
    if (gwave < a.n) fetch(gwave);
    for (uint64_t b = gwave; b < a.n; b += nwaves) {
        sx.store(img, lane); sy.store(img + G::SX, lane); sz.store(img + G::SX + G::SY, lane);
        skey.store(kimg, lane);
        const uint32_t lit_b = lit;
        wave_lds_sync();
        if (b + nwaves < a.n) fetch(b + nwaves);  // in flight while this block is checked
        block_unit_check(img, tab, t768, a.table, a.pt, a.ct, lit_b, ct_off, b, lane, acc);
        wave_lds_sync();  // the next block overwrites the image
    }
    flush_acc(a.report, acc);
    report_add(a.report + 7, off_bad);
}

// The report starts as (0 blocks, 0 keys, no failures, first = none, no offset failures): one eight-lane launch in front of the
// check instead of launch_check's two memsets.  One thing less to enqueue per call, and a kernel node replays the same in a
// captured graph as it runs eagerly; the 64-byte memset node this replaced left stale words behind on replay.
__global__ void __launch_bounds__(64) circ_report_init_kernel(uint64_t *report) {
    report_reset(report, 8, 1u << 6, threadIdx.x);
}

static hipError_t launch_circ_check(const CircCheckParams &p, bool dense, hipStream_t s) {
    hipLaunchKernelGGL(circ_report_init_kernel, dim3(1), dim3(64), 0, s, p.c.report);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds = check_lds_bytes(dense ? ChkLayout<DENSE>::IMG : ChkLayout<PACKED>::IMG);  // 41 / 46 KiB
    const uint64_t units = p.c.n > p.n_circuits ? p.c.n : p.n_circuits;  // n_circuits >= 1: there is always a key slab to check
    const dim3 grid((unsigned)check_groups(units)), block(CHECK_WAVES * LANES);
    if (dense) hipLaunchKernelGGL((circ_check_kernel<DENSE>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((circ_check_kernel<PACKED>), grid, block, lds, s, p);
    return hipGetLastError();
}

}  // namespace aesw_circ

extern "C" {

int aesw_circ_check_witness_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, uint64_t n,
                                   const uint8_t *d_pt, const uint8_t *d_keys, int layout, const uint8_t *d_x, const uint8_t *d_y,
                                   const uint8_t *d_z, const uint8_t *d_ct, const aesw_key_slab *d_key_slabs,
                                   aesw_circ_check_report *d_report, void *stream) {
    static_assert(sizeof(aesw_circ_check_report) == 8 * sizeof(uint64_t), "the kernel addresses the report as eight u64");
    if (int rc = aesw::entry_refused(ctx, "aesw_circ_check_witness_device")) return rc;
    if ((layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED) || k < 2 || k > 30 || n_sets == 0 || n_sets > 1024 ||
        n_circuits == 0 || !d_offsets || !aligned_to(d_offsets, 8) || !d_report || !aligned_to(d_report, 8))
        return AESW_ERR_INVALID_ARG;
    const aesw_key_slab *ks = d_key_slabs;
    if (!key_slab_ok(ks) || !aligned_to(d_keys, 4)) return AESW_ERR_INVALID_ARG;
    if (n && (!d_pt || !d_x || !d_y || !d_z || !aligned_to(d_pt, 4) || !aligned_to(d_ct, 4) || !aligned_to(d_x, 16) || !aligned_to(d_y, 16) ||
              !aligned_to(d_z, 16)))
        return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const int li = layout == AESW_LAYOUT_DENSE ? 0 : 1;  // the check tables were uploaded by aesw_create(): nothing is allocated here
    const aesw::CheckGeo cg = aesw::check_geo(layout);
    aesw_circ::CircCheckParams p{};
    p.c.pt = d_pt; p.c.keys = d_keys; p.c.x = d_x; p.c.y = d_y; p.c.z = d_z; p.c.ct = d_ct;
    aesw::set_key_slab(p.c, ks);
    p.c.table = ctx->d_chktab[li];
    p.c.tab768 = ctx->d_tables;
    p.c.report = reinterpret_cast<uint64_t *>(d_report);
    p.c.n = n;
    p.c.per_block_keys = 1;
    aesw::set_strides(p.c, aesw::slab_strides(layout));  // DENSE or PACKED (checked above): check_geo's domain
    p.c.bi = cg.bi;
    p.c.img = (cg.bi + cg.ki + 15u) & ~15u;
    p.offsets = d_offsets;
    p.cap = aesw_block_capacity(k, n_sets);
    p.n_circuits = n_circuits;
    HIP_TRY(ctx, aesw_circ::launch_circ_check(p, layout == AESW_LAYOUT_DENSE, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

uint32_t aesw_circ_circuit_of_block(const uint64_t *offsets, uint32_t n_circuits, uint64_t b) {
    if (!offsets || n_circuits == 0) return 0;
    return aesw_circ::circuit_of_block(offsets, n_circuits, b);
}

}  // extern "C"
