// aesw_hostpath.cpp -- the host-pointer entry points of include/aesw.h: they stage the caller's host buffers through the
// context's device scratch and call the device-pointer entry points of aesw_api.cpp.  Host code only.
// Pipeline: blocks are cut into chunks; chunk i's kernel runs on s_compute
// while chunk i-1's columns travel D2H on s_copy (two device buffer sets).
#include <hip/hip_runtime.h>
#include <sched.h>

#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/aesw.h"
#include "aesw_internal.h"
#include "aesw_check.h"

using namespace aesw;

#include "aesw_ctx.h"

// Pageable destinations: a stage arrives in the page-locked bounce buffer by DMA and is moved on from there by the CPU.  One
// thread moves ~20 GB/s (less into memory it touches for the first time), the link delivers 55: the move is cut into 4 MiB
// slices handed out to "copy_threads" threads (the caller is one of them).
int auto_copy_threads(const aesw_ctx *ctx) {
    if (ctx->opt.copy_threads >= 0) return ctx->opt.copy_threads < 1 ? 1 : ctx->opt.copy_threads;
    cpu_set_t set;
    int usable = 1;
    if (sched_getaffinity(0, sizeof set, &set) == 0) usable = CPU_COUNT(&set);
    // leave the host its cores: a quarter of what this process may run on, 1 ... 4, shared among the members of a group
    const int t = usable / (4 * ctx->group_size);
    return t < 1 ? 1 : (t > 4 ? 4 : t);
}

namespace {

struct CopyJob { uint8_t *dst; const uint8_t *src; size_t bytes; };

void parallel_copy(const std::vector<CopyJob> &jobs, int threads) noexcept {
    constexpr size_t SLICE = (size_t)4 << 20;
    std::vector<CopyJob> slices;
    std::vector<std::thread> pool;
    try {
        for (const CopyJob &j : jobs)
            for (size_t o = 0; o < j.bytes; o += SLICE) slices.push_back(CopyJob{j.dst + o, j.src + o, j.bytes - o < SLICE ? j.bytes - o : SLICE});
        pool.reserve(threads > 1 ? (size_t)threads - 1 : 0);
    } catch (...) {  // no memory for the bookkeeping: copy on this thread (nothing has been started yet)
        for (const CopyJob &j : jobs) std::memcpy(j.dst, j.src, j.bytes);
        return;
    }
    if ((int)slices.size() < threads) threads = (int)slices.size();
    std::atomic<size_t> next{0};
    auto work = [&]() noexcept {
        for (size_t i = next.fetch_add(1); i < slices.size(); i = next.fetch_add(1)) std::memcpy(slices[i].dst, slices[i].src, slices[i].bytes);
    };
    for (int t = 1; t < threads; ++t) {
        try { pool.emplace_back(work); } catch (...) { break; }  // no thread to be had: the others and the caller copy the rest
    }
    work();
    for (std::thread &t : pool) t.join();
}

struct DevBuf {
    uint8_t *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void **>(&p), n ? n : 16); }
};

int ensure_streams(aesw_ctx *ctx) {
    if (!ctx->s_compute) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_compute, hipStreamNonBlocking));
    if (!ctx->s_copy) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_copy, hipStreamNonBlocking));
    return AESW_OK;
}

bool is_pinned(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

int ensure_bounce(aesw_ctx *ctx, size_t bytes) {
    if (ctx->bounce_bytes >= bytes) return AESW_OK;
    for (int i = 0; i < 2; ++i) {
        if (ctx->bounce[i]) (void)hipHostFree(ctx->bounce[i]);
        ctx->bounce[i] = nullptr;
    }
    ctx->bounce_bytes = 0;
    for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->bounce[i]), bytes, hipHostMallocDefault));
    ctx->bounce_bytes = bytes;
    return AESW_OK;
}

int ensure_scratch(aesw_ctx *ctx, size_t bytes) {
    if (ctx->scratch_bytes >= bytes) return AESW_OK;
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->scratch), bytes));
    ctx->scratch_bytes = bytes;
    return AESW_OK;
}

// A buffer handed out in 256-byte-rounded pieces: the context's device scratch, or each of its two bounce buffers.
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};

// The grow-only buffers of the context, large enough for what a call has carved.
int ensure_carved(aesw_ctx *ctx, const Carve &dev, const Carve &host) {
    const int rc = ensure_scratch(ctx, dev.off);
    return rc != AESW_OK ? rc : ensure_bounce(ctx, host.off);
}

// Blocks per pipeline stage of a batch of n: "chunk_blocks", at most the batch, in whole 64-block units.
uint64_t stage_blocks(const aesw_ctx *ctx, uint64_t n) {
    const uint64_t chunk = (uint64_t)ctx->opt.chunk_blocks < n ? (uint64_t)ctx->opt.chunk_blocks : n;
    return (chunk + 63) / 64 * 64;
}

// ---- the two-stage pipeline ----------------------------------------------------------------------------------------
// One call's pipeline over the context's two streams.  The caller's items (chunks of blocks, or advice columns) alternate between
// stage 0 and stage 1: each stage has a piece of the device scratch and a bounce buffer of its own.  The entry point supplies two
// steps:
//   launch(s, first, count)             enqueue on s_compute whatever computes items [first, first + count) into stage s
//   copies(s, first, count, d2h, move)  name the D2H copies that stage needs, and for a copy that lands in the bounce buffer of
//                                       a call with a destination of its own, the CPU move that finishes it
struct Pipeline {
    aesw_ctx *ctx;
    bool timed = false;
    // per stage: kernel start / end, copy start / end (`started` and `copy0` only when timed: aesw_last_stream_stats)
    hipEvent_t started[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr}, copy0[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    uint64_t first[2] = {0, 0}, count[2] = {0, 0};  // the items a busy stage holds
    bool busy[2] = {false, false};
    std::vector<CopyJob> d2h, move[2];

    explicit Pipeline(aesw_ctx *c) : ctx(c) {}
    // Whatever happens, no copy may still be reading or writing the caller's buffers when the entry point returns.
    ~Pipeline() {
        for (hipEvent_t *v : {started, done, copy0, copied})
            for (int i = 0; i < 2; ++i)
                if (v[i]) (void)hipEventDestroy(v[i]);
        (void)hipStreamSynchronize(ctx->s_copy);
        (void)hipStreamSynchronize(ctx->s_compute);
    }

    int create_events(bool with_timing) {
        timed = with_timing;
        for (int i = 0; i < 2; ++i) {
            if (timed) {
                HIP_TRY(ctx, hipEventCreate(&started[i]));
                HIP_TRY(ctx, hipEventCreate(&done[i]));
                HIP_TRY(ctx, hipEventCreate(&copy0[i]));
                HIP_TRY(ctx, hipEventCreate(&copied[i]));
            } else {
                HIP_TRY(ctx, hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
                HIP_TRY(ctx, hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
            }
        }
        return AESW_OK;
    }

    template <class Launch, class Copies>
    int issue(int s, uint64_t b0, uint64_t m, Launch &launch, Copies &copies) {
        if (timed) HIP_TRY(ctx, hipEventRecord(started[s], ctx->s_compute));
        const int rc = launch(s, b0, m);
        if (rc != AESW_OK) return rc;
        HIP_TRY(ctx, hipEventRecord(done[s], ctx->s_compute));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_copy, done[s], 0));
        if (timed) HIP_TRY(ctx, hipEventRecord(copy0[s], ctx->s_copy));
        d2h.clear();
        move[s].clear();
        copies(s, b0, m, d2h, move[s]);
        for (const CopyJob &j : d2h) HIP_TRY(ctx, hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, ctx->s_copy));
        HIP_TRY(ctx, hipEventRecord(copied[s], ctx->s_copy));
        // no stream wait on copied[s] here: the next launch goes into the OTHER stage and may run while this one travels;
        // this stage is written again only after a driver below has host-synchronised copied[s]
        first[s] = b0; count[s] = m; busy[s] = true;
        return AESW_OK;
    }
};

// Drain-then-issue: the data ends in the caller's buffers.  Before stage s is reused, wait for its D2H and move what landed in
// its bounce buffer on to the (pageable) destination.
template <class Launch, class Copies>
int run_drain(Pipeline &pl, uint64_t n, uint64_t chunk, Launch launch, Copies copies) {
    auto drain = [&](int s) -> int {  // the device buffers and the bounce buffer of stage s are free again after this
        if (!pl.busy[s]) return AESW_OK;
        HIP_TRY(pl.ctx, hipEventSynchronize(pl.copied[s]));
        if (!pl.move[s].empty()) parallel_copy(pl.move[s], auto_copy_threads(pl.ctx));
        pl.busy[s] = false;
        return AESW_OK;
    };
    int s = 0;
    for (uint64_t b0 = 0; b0 < n; s ^= 1) {
        const uint64_t m = n - b0 < chunk ? n - b0 : chunk;
        int rc = drain(s);
        if (rc == AESW_OK) rc = pl.issue(s, b0, m, launch, copies);
        if (rc != AESW_OK) return rc;
        b0 += m;
    }
    const int rc = drain(s);  // the older stage first
    return rc != AESW_OK ? rc : drain(s ^ 1);
}

// Consume: two stages in flight; while the host consumes stage s out of its bounce buffer, stage s^1 is computed and copied.
// Accumulates the aesw_stream_stats of the call; a non-zero result of `consume(s, first, count)` ends it with AESW_ERR_MISMATCH.
template <class Launch, class Copies, class Consume>
int run_consume(Pipeline &pl, uint64_t n, uint64_t chunk, size_t bytes_per_item, Launch launch, Copies copies, Consume consume) {
    aesw_ctx *ctx = pl.ctx;
    aesw_stream_stats st = {};
    const uint64_t t_begin = now_ns();
    uint64_t b0 = 0;
    auto issue_next = [&](int s) -> int {
        if (b0 >= n) return AESW_OK;
        const uint64_t m = n - b0 < chunk ? n - b0 : chunk;
        const int rc = pl.issue(s, b0, m, launch, copies);
        b0 += m;
        return rc;
    };
    for (int s = 0; s < 2; ++s) {
        const int rc = issue_next(s);
        if (rc != AESW_OK) return rc;
    }
    for (int s = 0; pl.busy[s]; s ^= 1) {
        const uint64_t t0 = now_ns();
        HIP_TRY(ctx, hipEventSynchronize(pl.copied[s]));
        const uint64_t t1 = now_ns();
        pl.busy[s] = false;
        float ms = 0;
        if (hipEventElapsedTime(&ms, pl.started[s], pl.done[s]) == hipSuccess) st.kernel_ns += (uint64_t)(ms * 1e6);
        if (hipEventElapsedTime(&ms, pl.copy0[s], pl.copied[s]) == hipSuccess) st.d2h_ns += (uint64_t)(ms * 1e6);
        const int cr = consume(s, pl.first[s], pl.count[s]);
        const uint64_t t2 = now_ns();
        st.wait_ns += t1 - t0;
        st.consumer_ns += t2 - t1;
        st.chunks += 1;
        st.bytes_to_host += pl.count[s] * bytes_per_item;
        if (cr != 0) { st.wall_ns = now_ns() - t_begin; ctx->stats = st; return AESW_ERR_MISMATCH; }
        const int rc = issue_next(s);
        if (rc != AESW_OK) return rc;
    }
    st.wall_ns = now_ns() - t_begin;
    ctx->stats = st;
    return AESW_OK;
}

// ---- small shared pieces -------------------------------------------------------------------------------------------

// The four columns of `nk` key slabs between the host's slab (from its key `first` on) and a device slab; a column the host
// does not have is skipped.  Enqueued on `*s` if given, blocking copies otherwise.
int copy_key_slab(aesw_ctx *ctx, const aesw_key_slab &host, uint64_t first, const aesw_key_slab &dev, uint64_t nk, int layout,
                  hipMemcpyKind kind, const hipStream_t *s) {
    uint8_t *const h[4] = {host.w, host.kx, host.ky, host.kz}, *const d[4] = {dev.w, dev.kx, dev.ky, dev.kz};
    const SlabStrides st = slab_strides(layout);
    for (int c = 0; c < 4; ++c) {
        if (!h[c]) continue;
        const size_t stride = st[3 + c];  // w kx ky kz are columns 3..6 of the seven
        uint8_t *hp = h[c] + first * stride;
        void *dst = kind == hipMemcpyDeviceToHost ? hp : d[c];
        const void *src = kind == hipMemcpyDeviceToHost ? d[c] : hp;
        HIP_TRY(ctx, s ? hipMemcpyAsync(dst, src, nk * stride, kind, *s) : hipMemcpy(dst, src, nk * stride, kind));
    }
    return AESW_OK;
}
int key_slab_to_host(aesw_ctx *ctx, const aesw_key_slab &host, const aesw_key_slab &dev, uint64_t nk, int layout, const hipStream_t *s = nullptr) {
    return copy_key_slab(ctx, host, 0, dev, nk, layout, hipMemcpyDeviceToHost, s);
}
int key_slab_to_device(aesw_ctx *ctx, const aesw_key_slab &dev, const aesw_key_slab &host, uint64_t first, uint64_t nk, int layout) {
    return copy_key_slab(ctx, host, first, dev, nk, layout, hipMemcpyHostToDevice, nullptr);
}

}  // namespace

extern "C" {

int aesw_encrypt_witness(aesw_ctx *ctx, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n,
                         int layout, uint8_t *x, uint8_t *y, uint8_t *z, uint8_t *ct, const aesw_key_slab *ks) {
    if (aesw_is_group(ctx)) return aesw_group_encrypt_witness(ctx, pt, keys, per_block_keys, n, layout, x, y, z, ct, ks);
    if (!ctx || !aesw_valid_layout(layout)) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!pt) return AESW_ERR_INVALID_ARG;  // x / y / z: a null column is computed but not copied back
    if (!keys && (per_block_keys || (ks && (ks->w || ks->kx || ks->ky || ks->kz)))) return AESW_ERR_INVALID_ARG;
    if (!keys && !ctx->keys.has_key()) return AESW_ERR_NO_KEY;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    int rc = ensure_streams(ctx);
    if (rc != AESW_OK) return rc;
    const bool kemit = ks && (ks->w || ks->kx || ks->ky || ks->kz);
    const bool pbk = per_block_keys != 0;
    const uint64_t chunk = stage_blocks(ctx, n);

    // The seven output columns (x y z of the blocks; w kx ky kz of per-block keys): where chunk data goes and how.
    struct HostCol {
        uint8_t *dst;    // caller buffer (null = not wanted)
        size_t stride;   // bytes per block
        size_t doff[2];  // the stage's device buffer, inside the scratch
        bool direct;     // caller buffer is page-locked: DMA straight into it
        size_t boff;     // offset inside the bounce buffer
    } cols[7];
    const aesw_key_slab none{nullptr, nullptr, nullptr, nullptr}, &pks = pbk && kemit ? *ks : none;
    uint8_t *const dst[7] = {x, y, z, pks.w, pks.kx, pks.ky, pks.kz};
    // carve the context's device scratch: inputs, ciphertext, two sets of output columns
    Carve dev, host;
    const size_t o_pt = dev.take(n * 16), o_keys = dev.take(pbk ? n * 16 : 16), o_ct = dev.take(ct ? n * 16 : 0);
    const size_t kn = kemit ? (pbk ? chunk : 1) : 0;  // per-block keys: a key slab per block; shared key: one
    const SlabStrides st = slab_strides(layout);
    for (int c = 0; c < 7; ++c) cols[c].stride = st[c];
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 7; ++c) cols[c].doff[s] = dev.take((c < 3 ? chunk : kn) * cols[c].stride);
    for (int c = 0; c < 7; ++c) {
        HostCol &hc = cols[c];
        hc.dst = hc.stride ? dst[c] : nullptr;  // AESW_LAYOUT_VALUES has no x column
        hc.direct = hc.dst && is_pinned(hc.dst);
        hc.boff = hc.dst && !hc.direct ? host.take(chunk * hc.stride) : 0;
    }
    rc = ensure_carved(ctx, dev, host);
    if (rc != AESW_OK) return rc;
    uint8_t *d = ctx->scratch;
    auto slab_of = [&](int s) { return aesw_key_slab{d + cols[3].doff[s], d + cols[4].doff[s], d + cols[5].doff[s], d + cols[6].doff[s]}; };
    Pipeline pl(ctx);
    rc = pl.create_events(false);
    if (rc != AESW_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d + o_pt, pt, n * 16, hipMemcpyHostToDevice, ctx->s_compute));
    if (keys) HIP_TRY(ctx, hipMemcpyAsync(d + o_keys, keys, pbk ? n * 16 : 16, hipMemcpyHostToDevice, ctx->s_compute));

    if (!pbk && kemit) {
        // shared key: one key slab, staged in stage 0's (still unused) key buffers of the scratch, copied back on s_compute
        const aesw_key_slab one = slab_of(0);
        rc = aesw_key_schedule_witness_device(ctx, d + o_keys, 1, layout, one.w, one.kx, one.ky, one.kz, nullptr, ctx->s_compute);
        if (rc == AESW_OK) rc = key_slab_to_host(ctx, *ks, one, 1, layout, &ctx->s_compute);
        if (rc != AESW_OK) return rc;
    }

    auto launch = [&](int s, uint64_t b0, uint64_t m) -> int {
        const aesw_key_slab dks = slab_of(s);
        return aesw_encrypt_witness_device(ctx, d + o_pt + 16 * b0, !keys ? nullptr : (pbk ? d + o_keys + 16 * b0 : d + o_keys), per_block_keys, m,
                                           layout, d + cols[0].doff[s], d + cols[1].doff[s], d + cols[2].doff[s], ct ? d + o_ct + 16 * b0 : nullptr,
                                           pbk && kemit ? &dks : nullptr, ctx->s_compute);
    };
    auto copies = [&](int s, uint64_t b0, uint64_t m, std::vector<CopyJob> &d2h, std::vector<CopyJob> &move) {
        for (const HostCol &c : cols) {
            if (!c.dst) continue;
            uint8_t *fin = c.dst + b0 * c.stride, *to = c.direct ? fin : ctx->bounce[s] + c.boff;
            d2h.push_back(CopyJob{to, d + c.doff[s], (size_t)(m * c.stride)});
            if (!c.direct) move.push_back(CopyJob{fin, to, (size_t)(m * c.stride)});
        }
    };
    rc = run_drain(pl, n, chunk, launch, copies);
    if (rc != AESW_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_copy));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_compute));
    if (ct) HIP_TRY(ctx, hipMemcpy(ct, d + o_ct, n * 16, hipMemcpyDeviceToHost));
    return AESW_OK;
}

int aesw_encrypt_witness_stream(aesw_ctx *ctx, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout,
                                aesw_chunk_fn consume, void *user) {
    if (aesw_is_group(ctx)) return aesw_group_encrypt_witness_stream(ctx, pt, keys, per_block_keys, n, layout, consume, user);
    if (!ctx || !aesw_valid_layout(layout) || !consume) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!pt || (!keys && per_block_keys)) return AESW_ERR_INVALID_ARG;
    if (!keys && !ctx->keys.has_key()) return AESW_ERR_NO_KEY;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    int rc = ensure_streams(ctx);
    if (rc != AESW_OK) return rc;
    const SlabStrides st = slab_strides(layout);
    const bool pbk = per_block_keys != 0;
    const uint64_t chunk = stage_blocks(ctx, n);
    // device scratch: inputs + two sets of columns; page-locked bounce: two sets of columns
    Carve dev, host;
    size_t col_off[2][3], boff[3];
    const size_t o_pt = dev.take(n * 16), o_keys = dev.take(pbk ? n * 16 : 16);
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) col_off[s][c] = dev.take(chunk * st[c]);
    for (int c = 0; c < 3; ++c) boff[c] = host.take(chunk * st[c]);
    // "stream_check": every chunk is checked on the device behind its kernel (aesw_check.h).  Needs the key slab(s) the blocks' AddRoundKey
    // rows copy from -- one for a shared / scheduled key (made once, below), one per block with per-block keys (emitted by the chunk's
    // own launch into two more scratch sets) -- and one report per chunk, summed after the last one.
    const bool checking = ctx->opt.stream_check && layout != AESW_LAYOUT_VALUES;
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    size_t ks_off[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, o_rep = 0;
    if (checking) {
        const uint64_t nk = pbk ? chunk : 1;
        for (int s = 0; s < (pbk ? 2 : 1); ++s) {
            for (int c = 0; c < 4; ++c) ks_off[s][c] = dev.take(nk * st[3 + c]);  // w kx ky kz
        }
        if (!pbk) for (int c = 0; c < 4; ++c) ks_off[1][c] = ks_off[0][c];
        o_rep = dev.take(n_chunks * sizeof(aesw_check_report));
    }
    ctx->stream_report = aesw_check_report{0, 0, 0, 0, 0, 0, AESW_CHECK_NONE};
    rc = ensure_carved(ctx, dev, host);
    if (rc != AESW_OK) return rc;
    uint8_t *d = ctx->scratch;
    Pipeline pl(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(d + o_pt, pt, n * 16, hipMemcpyHostToDevice, ctx->s_compute));
    if (keys) HIP_TRY(ctx, hipMemcpyAsync(d + o_keys, keys, pbk ? n * 16 : 16, hipMemcpyHostToDevice, ctx->s_compute));
    auto slab_of = [&](int s) { return aesw_key_slab{d + ks_off[s][0], d + ks_off[s][1], d + ks_off[s][2], d + ks_off[s][3]}; };
    const uint8_t *d_key16 = nullptr;  // the 16 key bytes of a shared / scheduled key on the device (the literal rows of words_column)
    KeyRing::Access key_read;          // of a scheduled key, read by the key-slab launch below and by every chunk's check
    if (checking && !pbk) {
        // a scheduled key's bytes are the first round key of its slot (rk[0] = the key, src/key_schedule.rs:107-114)
        // (the context's own stream is never captured: an eager read, one wait for a key written on another stream)
        if (!keys && (rc = ctx->keys.begin_read(ctx, ctx->s_compute, &key_read)) != AESW_OK) return rc;
        d_key16 = keys ? d + o_keys : key_read.d;
        const aesw_key_slab one = slab_of(0);
        KeyParams kp{d_key16, ctx->d_tables, KeyOut{one.w, one.kx, one.ky, one.kz}, nullptr, 1, 0, 0};
        HIP_TRY(ctx, launch_key(kp, layout, ctx->xt, 1, ctx->opt.key_nt, 0u, ctx->s_compute));
        if (!keys && (rc = ctx->keys.end_read(ctx, key_read)) != AESW_OK) return rc;
    }
    rc = pl.create_events(true);  // timed: aesw_last_stream_stats reports where the time went
    if (rc != AESW_OK) return rc;
    auto launch = [&](int s, uint64_t b0, uint64_t m) -> int {
        const aesw_key_slab stage_slab = slab_of(s);
        int r = aesw_encrypt_witness_device(ctx, d + o_pt + 16 * b0, !keys ? nullptr : (pbk ? d + o_keys + 16 * b0 : d + o_keys), per_block_keys, m,
                                            layout, d + col_off[s][0], d + col_off[s][1], d + col_off[s][2], nullptr,
                                            checking && pbk ? &stage_slab : nullptr, ctx->s_compute);
        if (r != AESW_OK) return r;
        if (ctx->opt.stream_poison > 0 && (uint64_t)ctx->opt.stream_poison - 1 >= b0 && (uint64_t)ctx->opt.stream_poison - 1 < b0 + m) {
            // diagnostic: two cells of one block are overwritten between the kernel and the check (tests/test_gpu_round4.py shows the
            // stream check names that block, by its batch-wide index, in whatever chunk it lies)
            const uint64_t pb = (uint64_t)ctx->opt.stream_poison - 1 - b0;
            HIP_TRY(ctx, hipMemsetAsync(d + col_off[s][1] + pb * st[1] + 5, 0x5A, 1, ctx->s_compute));
            HIP_TRY(ctx, hipMemsetAsync(d + col_off[s][2] + pb * st[2] + 7, 0xA5, 1, ctx->s_compute));
        }
        if (!checking) return AESW_OK;
        r = check_witness_impl(ctx, d + o_pt + 16 * b0, pbk ? d + o_keys + 16 * b0 : d_key16, per_block_keys, m, layout, d + col_off[s][0],
                               d + col_off[s][1], d + col_off[s][2], nullptr, &stage_slab,
                               reinterpret_cast<aesw_check_report *>(d + o_rep) + b0 / chunk, ctx->s_compute, !pbk && b0 != 0);
        if (r != AESW_OK || keys) return r;
        return ctx->keys.end_read(ctx, key_read);  // the check read the slot, on the stream key_read was begun on
    };
    auto copies = [&](int s, uint64_t, uint64_t m, std::vector<CopyJob> &d2h, std::vector<CopyJob> &) {
        for (int c = 0; c < 3; ++c)
            if (st[c]) d2h.push_back(CopyJob{ctx->bounce[s] + boff[c], d + col_off[s][c], (size_t)(m * st[c])});
    };
    auto hand_over = [&](int s, uint64_t first, uint64_t count) {
        return consume(user, first, count, st[0] ? ctx->bounce[s] + boff[0] : nullptr /* AESW_LAYOUT_VALUES: no x */,
                       ctx->bounce[s] + boff[1], ctx->bounce[s] + boff[2]);
    };
    rc = run_consume(pl, n, chunk, st.block_bytes(), launch, copies, hand_over);
    if (rc != AESW_OK) return rc;
    if (checking) {  // every chunk's kernel and check have finished (their columns have been copied): sum the reports
        std::vector<aesw_check_report> reps((size_t)n_chunks);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->s_compute));  // (a non-blocking stream: the copy below does not wait for it by itself)
        HIP_TRY(ctx, hipMemcpy(reps.data(), d + o_rep, reps.size() * sizeof(aesw_check_report), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n_chunks; ++i) merge_check_report(ctx->stream_report, reps[i], i * chunk, pbk);
    }
    return AESW_OK;
}

int aesw_last_stream_check(const aesw_ctx *ctx, aesw_check_report *out) {
    if (!ctx || !out) return AESW_ERR_INVALID_ARG;
    *out = ctx->stream_report;
    return AESW_OK;
}

int aesw_last_stream_stats(const aesw_ctx *ctx, aesw_stream_stats *out) {
    if (!ctx || !out) return AESW_ERR_INVALID_ARG;
    *out = ctx->stats;
    return AESW_OK;
}

// Whole advice columns of a K/N circuit to the host, column by column ("the host can bulk-copy into
// halo2's advice polynomials"): column j is assembled on s_compute into one of two device buffers and travels D2H on s_copy
// while column j+1 is assembled.  `stream` hands each column to `consume` out of one of two page-locked buffers; `host` puts
// them straight into ONE host buffer (column after column): DMA directly when the buffer is page-locked (aesw_host_alloc, or the
// host's own advice-polynomial memory after aesw_host_register), through the bounce buffers otherwise.
// The caller's slabs were produced on some stream of theirs: they must be complete before the call (documented).
static int assemble_columns(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x, const uint8_t *d_y,
                            const uint8_t *d_z, const aesw_key_slab *ks, int as_fr, aesw_column_fn consume, void *user, uint8_t *out) {
    AssembleParams p;
    int rc = fill_assemble_params(ctx, k, n_sets, n_blocks, layout, d_x, d_y, d_z, ks, &p);
    if (rc != AESW_OK) return rc;
    if (k > 28) return AESW_ERR_INVALID_ARG;  // one column must fit the staging buffers
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    rc = ensure_streams(ctx);
    if (rc != AESW_OK) return rc;
    const uint64_t rows = (uint64_t)1 << k;
    const size_t col_bytes = (size_t)rows * (as_fr ? AESW_FR_BYTES : 1);
    const uint32_t ncols = 3 * n_sets + 1;
    const bool direct = out && is_pinned(out) && is_pinned(out + (size_t)ncols * col_bytes - 1);
    Carve dev, host;
    const size_t slot[2] = {dev.take(col_bytes), dev.take(col_bytes)};
    if (!direct) host.take(col_bytes);
    rc = ensure_carved(ctx, dev, host);
    if (rc != AESW_OK) return rc;
    Pipeline pl(ctx);
    rc = pl.create_events(consume != nullptr);
    if (rc != AESW_OK) return rc;
    auto launch = [&](int s, uint64_t col, uint64_t) -> int {
        AssembleParams q = p;
        q.col_first = (uint32_t)col;
        q.col_count = 1;
        q.out = ctx->scratch + slot[s];
        HIP_TRY(ctx, launch_assemble(q, as_fr != 0, ctx->opt.fr_nt, ctx->s_compute));
        return AESW_OK;
    };
    auto copies = [&](int s, uint64_t col, uint64_t, std::vector<CopyJob> &d2h, std::vector<CopyJob> &move) {
        uint8_t *fin = out ? out + (size_t)col * col_bytes : nullptr, *to = direct ? fin : ctx->bounce[s];
        d2h.push_back(CopyJob{to, ctx->scratch + slot[s], col_bytes});
        if (out && !direct) move.push_back(CopyJob{fin, to, col_bytes});
    };
    if (out) return run_drain(pl, ncols, 1, launch, copies);
    return run_consume(pl, ncols, 1, col_bytes, launch, copies,
                       [&](int s, uint64_t col, uint64_t) { return consume(user, (uint32_t)col, ctx->bounce[s], rows); });
}

int aesw_assemble_advice_stream(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x,
                                const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *ks, int as_fr, aesw_column_fn consume,
                                void *user) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_assemble_advice_stream");
    if (!consume) return AESW_ERR_INVALID_ARG;
    return assemble_columns(ctx, k, n_sets, n_blocks, layout, d_x, d_y, d_z, ks, as_fr, consume, user, nullptr);
}

int aesw_assemble_advice_host(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x,
                              const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *ks, int as_fr, uint8_t *out) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_assemble_advice_host");
    if (!out) return AESW_ERR_INVALID_ARG;
    return assemble_columns(ctx, k, n_sets, n_blocks, layout, d_x, d_y, d_z, ks, as_fr, nullptr, nullptr, out);
}

int aesw_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return AESW_ERR_INVALID_ARG;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return AESW_ERR_HIP;
    }
    return AESW_OK;
}

int aesw_host_unregister(void *p) {
    if (!p) return AESW_ERR_INVALID_ARG;
    if (hipHostUnregister(p) != hipSuccess) {
        (void)hipGetLastError();
        return AESW_ERR_HIP;
    }
    return AESW_OK;
}

int aesw_key_schedule_witness(aesw_ctx *ctx, const uint8_t *keys, uint64_t n, int layout, uint8_t *w, uint8_t *kx,
                              uint8_t *ky, uint8_t *kz, uint8_t *rk) {
    if (aesw_is_group(ctx)) return aesw_group_key_schedule_witness(ctx, keys, n, layout, w, kx, ky, kz, rk);
    if (!ctx || !aesw_valid_layout(layout)) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!keys) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    DevBuf dk, dw, dkx, dky, dkz, drk;
    HIP_TRY(ctx, dk.alloc(n * 16));
    const SlabStrides st = slab_strides(layout);
    if (w) HIP_TRY(ctx, dw.alloc(n * st.words));
    if (kx) HIP_TRY(ctx, dkx.alloc(n * st.kx));
    if (ky) HIP_TRY(ctx, dky.alloc(n * st.ky));
    if (kz) HIP_TRY(ctx, dkz.alloc(n * st.kz));
    if (rk) HIP_TRY(ctx, drk.alloc(n * RK_BYTES));
    HIP_TRY(ctx, hipMemcpy(dk.p, keys, n * 16, hipMemcpyHostToDevice));
    int rc = aesw_key_schedule_witness_device(ctx, dk.p, n, layout, dw.p, dkx.p, dky.p, dkz.p, drk.p, nullptr);  // (not allocated = null = not wanted)
    if (rc != AESW_OK) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    rc = key_slab_to_host(ctx, aesw_key_slab{w, kx, ky, kz}, aesw_key_slab{dw.p, dkx.p, dky.p, dkz.p}, n, layout);
    if (rc != AESW_OK) return rc;
    if (rk) HIP_TRY(ctx, hipMemcpy(rk, drk.p, n * RK_BYTES, hipMemcpyDeviceToHost));
    return AESW_OK;
}

int aesw_check_witness(aesw_ctx *ctx, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout, const uint8_t *x,
                       const uint8_t *y, const uint8_t *z, const uint8_t *ct, const aesw_key_slab *ks, aesw_check_report *report) {
    if (aesw_is_group(ctx)) return aesw_group_check_witness(ctx, pt, keys, per_block_keys, n, layout, x, y, z, ct, ks, report);
    if (!ctx || !report || (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED)) return AESW_ERR_INVALID_ARG;
    if (per_block_keys && n && !keys) return AESW_ERR_INVALID_ARG;
    if (n && (!pt || !x || !y || !z || !ks || !ks->w || !ks->kx || !ks->ky || !ks->kz)) return AESW_ERR_INVALID_ARG;
    *report = aesw_check_report{0, 0, 0, 0, 0, 0, AESW_CHECK_NONE};
    if (n == 0) return AESW_OK;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const CheckGeo cg = check_geo(layout);
    const uint64_t chunk = (uint64_t)ctx->opt.chunk_blocks < n ? (uint64_t)ctx->opt.chunk_blocks : n;
    const uint64_t nk = per_block_keys ? chunk : 1;
    DevBuf dpt, dkeys, dx, dy, dz, dct, dw, dkx, dky, dkz, drep;
    HIP_TRY(ctx, dpt.alloc(chunk * 16));
    HIP_TRY(ctx, dkeys.alloc(nk * 16));
    HIP_TRY(ctx, dx.alloc(chunk * cg.sx)); HIP_TRY(ctx, dy.alloc(chunk * cg.sy)); HIP_TRY(ctx, dz.alloc(chunk * cg.sz));
    HIP_TRY(ctx, dct.alloc(chunk * 16));
    HIP_TRY(ctx, dw.alloc(nk * WORDS_ROWS)); HIP_TRY(ctx, dkx.alloc(nk * cg.kxs)); HIP_TRY(ctx, dky.alloc(nk * cg.kys)); HIP_TRY(ctx, dkz.alloc(nk * cg.kzs));
    HIP_TRY(ctx, drep.alloc(sizeof(aesw_check_report)));
    const aesw_key_slab dks{dw.p, dkx.p, dky.p, dkz.p};
    if (!per_block_keys) {  // the one key slab of the batch travels once
        if (keys) HIP_TRY(ctx, hipMemcpy(dkeys.p, keys, 16, hipMemcpyHostToDevice));
        const int rc = key_slab_to_device(ctx, dks, *ks, 0, 1, layout);
        if (rc != AESW_OK) return rc;
    }
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t m = n - lo < chunk ? n - lo : chunk;
        HIP_TRY(ctx, hipMemcpy(dpt.p, pt + lo * 16, m * 16, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(dx.p, x + lo * cg.sx, m * cg.sx, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(dy.p, y + lo * cg.sy, m * cg.sy, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(dz.p, z + lo * cg.sz, m * cg.sz, hipMemcpyHostToDevice));
        if (ct) HIP_TRY(ctx, hipMemcpy(dct.p, ct + lo * 16, m * 16, hipMemcpyHostToDevice));
        int rc = AESW_OK;
        if (per_block_keys) {
            HIP_TRY(ctx, hipMemcpy(dkeys.p, keys + lo * 16, m * 16, hipMemcpyHostToDevice));
            rc = key_slab_to_device(ctx, dks, *ks, lo, m, layout);
        }
        if (rc == AESW_OK)
            rc = check_witness_impl(ctx, dpt.p, (per_block_keys || keys) ? dkeys.p : nullptr, per_block_keys, m, layout, dx.p, dy.p, dz.p,
                                    ct ? dct.p : nullptr, &dks, reinterpret_cast<aesw_check_report *>(drep.p), nullptr,
                                    /* skip the shared key slab */ !per_block_keys && lo != 0);
        if (rc != AESW_OK) return rc;
        aesw_check_report r;
        HIP_TRY(ctx, hipMemcpy(&r, drep.p, sizeof r, hipMemcpyDeviceToHost));  // (synchronises with the null stream's launch)
        merge_check_report(*report, r, lo, per_block_keys != 0);
    }
    return AESW_OK;
}

int aesw_schedule_key(aesw_ctx *ctx, const uint8_t key[16], int layout, const aesw_key_slab *ks) {
    if (aesw_is_group(ctx)) return aesw_group_schedule_key(ctx, key, layout, ks);
    if (!ctx || !aesw_valid_layout(layout) || !key) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    DevBuf dk, dw, dkx, dky, dkz;
    HIP_TRY(ctx, dk.alloc(16));
    const SlabStrides st = slab_strides(layout);
    HIP_TRY(ctx, dw.alloc(st.words));
    HIP_TRY(ctx, dkx.alloc(st.kx));
    HIP_TRY(ctx, dky.alloc(st.ky));
    HIP_TRY(ctx, dkz.alloc(st.kz));
    HIP_TRY(ctx, hipMemcpy(dk.p, key, 16, hipMemcpyHostToDevice));
    aesw_key_slab dks{dw.p, dkx.p, dky.p, dkz.p};
    int rc = aesw_schedule_key_device(ctx, dk.p, layout, ks ? &dks : nullptr, nullptr);
    if (rc != AESW_OK) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    return ks ? key_slab_to_host(ctx, *ks, dks, 1, layout) : AESW_OK;
}

void *aesw_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void aesw_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int aesw_lookup_table(aesw_ctx *ctx, uint8_t *t0, uint8_t *t1, uint8_t *t2, uint8_t *t3) {
    if (aesw_is_group(ctx)) return aesw_group_lookup_table(ctx, t0, t1, t2, t3);
    if (!ctx || !t0 || !t1 || !t2 || !t3) return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    DevBuf d;
    HIP_TRY(ctx, d.alloc(4 * (size_t)AESW_TABLE_ROWS));
    uint8_t *p = d.p;
    int rc = aesw_lookup_table_device(ctx, p, p + AESW_TABLE_ROWS, p + 2 * (size_t)AESW_TABLE_ROWS,
                                      p + 3 * (size_t)AESW_TABLE_ROWS, nullptr);
    if (rc != AESW_OK) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());
    uint8_t *outs[4] = {t0, t1, t2, t3};
    for (int i = 0; i < 4; ++i)
        HIP_TRY(ctx, hipMemcpy(outs[i], p + i * (size_t)AESW_TABLE_ROWS, AESW_TABLE_ROWS, hipMemcpyDeviceToHost));
    return AESW_OK;
}

}  // extern "C"
