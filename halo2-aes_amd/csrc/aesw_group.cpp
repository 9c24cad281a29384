// aesw_group.cpp -- group contexts (include/aesw.h "device groups"): one aesw_ctx that owns a member context per listed device.
// The host-pointer entry points split a batch into contiguous block shards [n*i/G, n*(i+1)/G) (sharding.shard_range); member i runs
// its shard through the plain entry point on a host thread of its own, so every GPU moves its shard over its own link straight into
// the caller's buffers.  No kernel and no device memory of its own: a member is an ordinary context.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aesw.h"
#include "aesw_ctx.h"
#include "aesw_slabmap.h"

namespace {

constexpr uint32_t MAX_MEMBERS = 64;

void shard_of(uint32_t members, uint64_t n, uint32_t i, uint64_t *first, uint64_t *count) {
    const unsigned __int128 lo = (unsigned __int128)n * i / members, hi = (unsigned __int128)n * (i + 1) / members;
    *first = (uint64_t)lo;
    *count = (uint64_t)(hi - lo);
}

template <class T>
T *at(T *p, uint64_t off) { return p ? p + off : nullptr; }

uint32_t size_of(const aesw_ctx *g) { return (uint32_t)g->members.size(); }

// the group's status: the first non-OK one in member order, and aesw_last_error(group) names that member and its device
int first_failure(aesw_ctx *g, const std::vector<int> &status, const std::vector<char> *ignore = nullptr) {
    for (uint32_t i = 0; i < status.size(); ++i) {
        if (status[i] == AESW_OK || (ignore && (*ignore)[i])) continue;
        const aesw_ctx *m = g->members[i];
        char buf[512];
        std::snprintf(buf, sizeof buf, "member %u (device %d): %s%s%s", i, m->device, aesw_strerror(status[i]),
                      m->last_error.empty() ? "" : ": ", m->last_error.c_str());
        g->last_error = buf;
        return status[i];
    }
    return AESW_OK;
}

// fn(i) for every member: member 0 on the calling thread, the others on threads of their own (on the calling thread after member 0
// when no thread can be had).  Returns after every member has finished.
int run_members(aesw_ctx *g, const std::function<int(uint32_t)> &fn) {
    const uint32_t G = size_of(g);
    std::vector<int> status(G, AESW_OK);
    std::vector<char> inline_run(G, 0);
    std::vector<std::thread> pool;
    for (aesw_ctx *m : g->members) m->last_error.clear();  // what a member reports below is about this call
    try { pool.reserve(G); } catch (...) {}
    for (uint32_t i = 1; i < G; ++i) {
        try {
            pool.emplace_back([&, i]() noexcept { status[i] = fn(i); });
        } catch (...) {
            inline_run[i] = 1;
        }
    }
    status[0] = fn(0);
    for (uint32_t i = 1; i < G; ++i)
        if (inline_run[i]) status[i] = fn(i);
    for (std::thread &t : pool) t.join();
    return first_failure(g, status);
}

// aesw_encrypt_witness_stream: members hand their chunks to the calling thread, which runs `consume` one chunk at a time
struct StreamHub {
    struct Chunk {
        uint64_t first, count;
        const uint8_t *x, *y, *z;
        int result;
        bool done;
    };
    std::mutex mu;
    std::condition_variable to_caller, to_members;
    std::deque<Chunk *> ready;
    uint32_t running = 0;  // members whose stream call has not returned
    bool stop = false;     // every member stops at its next chunk boundary
    bool refused = false;  // ... because `consume` returned non-zero
};
struct MemberFeed {
    StreamHub *hub;
    uint64_t offset;       // the member's first block in the batch
    bool stopped = false;  // the member's stream ended because the group stopped, not by a failure of its own
};

int feed_chunk(void *user, uint64_t first_block, uint64_t n_blocks, const uint8_t *x, const uint8_t *y, const uint8_t *z) {
    MemberFeed &f = *static_cast<MemberFeed *>(user);
    StreamHub &h = *f.hub;
    std::unique_lock<std::mutex> lk(h.mu);
    if (h.stop) { f.stopped = true; return 1; }
    StreamHub::Chunk c{f.offset + first_block, n_blocks, x, y, z, 0, false};
    h.ready.push_back(&c);
    h.to_caller.notify_one();
    h.to_members.wait(lk, [&] { return c.done; });  // the buffers stay valid until the consumer has returned
    if (c.result != 0) f.stopped = true;
    return c.result;
}

}  // namespace

int aesw_group_refuse(aesw_ctx *g, const char *entry) {
    g->last_error = std::string(entry) + ": a group context has no device-pointer, column-arena, assemble or communicator entry points "
                                         "(device pointers belong to one GPU); call it on a member (aesw_group_member)";
    return AESW_ERR_INVALID_ARG;
}

void aesw_group_destroy(aesw_ctx *g) {
    for (aesw_ctx *m : g->members) aesw_destroy(m);
    delete g;
}

int aesw_group_set_option(aesw_ctx *g, const char *name, int64_t value) {
    std::vector<int> status(size_of(g), AESW_OK);
    for (uint32_t i = 0; i < size_of(g); ++i) status[i] = aesw_set_option(g->members[i], name, value);
    return first_failure(g, status);
}

int aesw_group_encrypt_witness(aesw_ctx *g, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout, uint8_t *x,
                               uint8_t *y, uint8_t *z, uint8_t *ct, const aesw_key_slab *ks) {
    // the plain entry point's own argument checks, before anything is split, so that the status does not depend on the shards
    if (!aesw_valid_layout(layout)) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!pt) return AESW_ERR_INVALID_ARG;
    const bool kemit = ks && (ks->w || ks->kx || ks->ky || ks->kz);
    if (!keys && (per_block_keys || kemit)) return AESW_ERR_INVALID_ARG;
    const uint32_t G = size_of(g);
    const bool pbk = per_block_keys != 0;
    const aesw::SlabStrides st = aesw::slab_strides(layout);
    // a shared key's one slab is written by the first member that has blocks (member 0 whenever n >= G)
    uint32_t slab_member = 0;
    for (uint64_t b0, m; slab_member < G; ++slab_member) {
        shard_of(G, n, slab_member, &b0, &m);
        if (m) break;
    }
    return run_members(g, [&](uint32_t i) -> int {
        uint64_t b0, m;
        shard_of(G, n, i, &b0, &m);
        if (m == 0) return AESW_OK;
        aesw_key_slab own{nullptr, nullptr, nullptr, nullptr};
        if (kemit && pbk) own = aesw_key_slab{at(ks->w, b0 * st.words), at(ks->kx, b0 * st.kx), at(ks->ky, b0 * st.ky), at(ks->kz, b0 * st.kz)};
        else if (kemit && i == slab_member) own = *ks;
        return aesw_encrypt_witness(g->members[i], pt + 16 * b0, pbk ? keys + 16 * b0 : keys, per_block_keys, m, layout, at(x, b0 * st.x),
                                    at(y, b0 * st.y), at(z, b0 * st.z), at(ct, 16 * b0), &own);
    });
}

int aesw_group_encrypt_witness_stream(aesw_ctx *g, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout,
                                      aesw_chunk_fn consume, void *user) {
    if (!aesw_valid_layout(layout) || !consume) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!pt || (!keys && per_block_keys)) return AESW_ERR_INVALID_ARG;
    const uint32_t G = size_of(g);
    const bool pbk = per_block_keys != 0;
    const uint64_t t_begin = now_ns();
    StreamHub hub;
    std::vector<MemberFeed> feed(G, MemberFeed{&hub, 0});
    std::vector<uint64_t> first(G), count(G);
    std::vector<int> status(G, AESW_OK);
    for (uint32_t i = 0; i < G; ++i) {
        shard_of(G, n, i, &first[i], &count[i]);
        feed[i].offset = first[i];
        aesw_ctx *m = g->members[i];
        m->last_error.clear();
        m->stats = aesw_stream_stats{};
        m->stream_report = aesw_check_report{0, 0, 0, 0, 0, 0, AESW_CHECK_NONE};
    }
    auto work = [&](uint32_t i) noexcept {
        int rc = AESW_OK;
        if (count[i])
            rc = aesw_encrypt_witness_stream(g->members[i], pt + 16 * first[i], pbk ? keys + 16 * first[i] : keys, per_block_keys, count[i],
                                             layout, feed_chunk, &feed[i]);
        std::lock_guard<std::mutex> lk(hub.mu);
        status[i] = rc;
        if (rc != AESW_OK && !feed[i].stopped) hub.stop = true;  // a member's own failure stops the others too
        --hub.running;
        hub.to_caller.notify_one();
    };
    // every member on a thread of its own: the calling thread is the consumer's
    std::vector<std::thread> pool;
    try { pool.reserve(G); } catch (...) {}
    {
        std::lock_guard<std::mutex> lk(hub.mu);
        hub.running = G;
    }
    for (uint32_t i = 0; i < G; ++i) {
        try {
            pool.emplace_back(work, i);
        } catch (...) {
            std::lock_guard<std::mutex> lk(hub.mu);
            status[i] = AESW_ERR_NOMEM;
            hub.stop = true;
            --hub.running;
        }
    }
    {
        std::unique_lock<std::mutex> lk(hub.mu);
        for (;;) {
            hub.to_caller.wait(lk, [&] { return !hub.ready.empty() || hub.running == 0; });
            if (hub.ready.empty()) break;
            StreamHub::Chunk *c = hub.ready.front();
            hub.ready.pop_front();
            int r = 1;  // a chunk that was waiting when the group stopped is not delivered
            if (!hub.stop) {
                lk.unlock();
                r = consume(user, c->first, c->count, c->x, c->y, c->z);
                lk.lock();
                if (r != 0) { hub.stop = true; hub.refused = true; }
            }
            c->result = r;
            c->done = true;
            hub.to_members.notify_all();
        }
    }
    for (std::thread &t : pool) t.join();
    aesw_stream_stats st = {};
    aesw_check_report rep = {0, 0, 0, 0, 0, 0, AESW_CHECK_NONE};
    for (uint32_t i = 0; i < G; ++i) {
        if (!count[i]) continue;
        const aesw_ctx *m = g->members[i];
        st.chunks += m->stats.chunks; st.bytes_to_host += m->stats.bytes_to_host;
        st.kernel_ns += m->stats.kernel_ns; st.d2h_ns += m->stats.d2h_ns;
        st.consumer_ns += m->stats.consumer_ns; st.wait_ns += m->stats.wait_ns;
        merge_check_report(rep, m->stream_report, first[i], pbk);
    }
    st.wall_ns = now_ns() - t_begin;
    g->stats = st;
    g->stream_report = rep;
    if (hub.refused) return AESW_ERR_MISMATCH;
    std::vector<char> stopped(G);
    for (uint32_t i = 0; i < G; ++i) stopped[i] = feed[i].stopped ? 1 : 0;
    return first_failure(g, status, &stopped);
}

int aesw_group_key_schedule_witness(aesw_ctx *g, const uint8_t *keys, uint64_t n, int layout, uint8_t *w, uint8_t *kx, uint8_t *ky, uint8_t *kz,
                                    uint8_t *rk) {
    if (!aesw_valid_layout(layout)) return AESW_ERR_INVALID_ARG;
    if (n == 0) return AESW_OK;
    if (!keys) return AESW_ERR_INVALID_ARG;
    const uint32_t G = size_of(g);
    const aesw::SlabStrides st = aesw::slab_strides(layout);
    return run_members(g, [&](uint32_t i) -> int {
        uint64_t k0, m;
        shard_of(G, n, i, &k0, &m);
        if (m == 0) return AESW_OK;
        return aesw_key_schedule_witness(g->members[i], keys + 16 * k0, m, layout, at(w, k0 * st.words), at(kx, k0 * st.kx), at(ky, k0 * st.ky),
                                         at(kz, k0 * st.kz), at(rk, k0 * aesw::RK_BYTES));
    });
}

int aesw_group_check_witness(aesw_ctx *g, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout, const uint8_t *x,
                             const uint8_t *y, const uint8_t *z, const uint8_t *ct, const aesw_key_slab *ks, aesw_check_report *report) {
    if (!report || (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED)) return AESW_ERR_INVALID_ARG;
    if (per_block_keys && n && !keys) return AESW_ERR_INVALID_ARG;
    if (n && (!pt || !x || !y || !z || !ks || !ks->w || !ks->kx || !ks->ky || !ks->kz)) return AESW_ERR_INVALID_ARG;
    *report = aesw_check_report{0, 0, 0, 0, 0, 0, AESW_CHECK_NONE};
    if (n == 0) return AESW_OK;
    const uint32_t G = size_of(g);
    const bool pbk = per_block_keys != 0;
    const aesw::SlabStrides st = aesw::slab_strides(layout);
    std::vector<aesw_check_report> reps(G, aesw_check_report{0, 0, 0, 0, 0, 0, AESW_CHECK_NONE});
    std::vector<uint64_t> first(G), count(G);
    for (uint32_t i = 0; i < G; ++i) shard_of(G, n, i, &first[i], &count[i]);
    const int rc = run_members(g, [&](uint32_t i) -> int {
        const uint64_t b0 = first[i], m = count[i];
        if (m == 0) return AESW_OK;
        // per-block keys: the member's own key slabs; a shared key: its one slab goes to every member
        const aesw_key_slab own = pbk ? aesw_key_slab{ks->w + b0 * st.words, ks->kx + b0 * st.kx, ks->ky + b0 * st.ky, ks->kz + b0 * st.kz} : *ks;
        return aesw_check_witness(g->members[i], pt + 16 * b0, pbk ? keys + 16 * b0 : keys, per_block_keys, m, layout, x + b0 * st.x, y + b0 * st.y,
                                  z + b0 * st.z, at(ct, 16 * b0), &own, &reps[i]);
    });
    if (rc != AESW_OK) return rc;
    for (uint32_t i = 0; i < G; ++i)
        if (count[i]) merge_check_report(*report, reps[i], first[i], pbk);
    return AESW_OK;
}

int aesw_group_schedule_key(aesw_ctx *g, const uint8_t key[16], int layout, const aesw_key_slab *ks) {
    if (!aesw_valid_layout(layout) || !key) return AESW_ERR_INVALID_ARG;
    // every member holds the key for its later scheduled-key calls; member 0 writes the optional key slab
    return run_members(g, [&](uint32_t i) -> int { return aesw_schedule_key(g->members[i], key, layout, i == 0 ? ks : nullptr); });
}

int aesw_group_lookup_table(aesw_ctx *g, uint8_t *t0, uint8_t *t1, uint8_t *t2, uint8_t *t3) {
    std::vector<int> status(size_of(g), AESW_OK);
    status[0] = aesw_lookup_table(g->members[0], t0, t1, t2, t3);
    return first_failure(g, status);
}

extern "C" {

int aesw_group_shard(uint32_t members, uint64_t n, uint32_t i, uint64_t *first, uint64_t *count) {
    if (members == 0 || i >= members || !first || !count) return AESW_ERR_INVALID_ARG;
    shard_of(members, n, i, first, count);
    return AESW_OK;
}

int aesw_create_group(aesw_ctx **out, const int *devices, uint32_t count, const uint8_t sbox[256], const uint8_t mul2[256],
                      const uint8_t mul3[256]) {
    if (!out) return AESW_ERR_INVALID_ARG;
    *out = nullptr;
    if (!sbox || !mul2 || !mul3) return AESW_ERR_INVALID_ARG;
    if (devices && (count == 0 || count > MAX_MEMBERS)) return AESW_ERR_INVALID_ARG;
    std::vector<int> devs;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return AESW_ERR_NO_DEVICE;
    try {
        if (devices) devs.assign(devices, devices + count);
        else for (int d = 0; d < n_dev && d < (int)MAX_MEMBERS; ++d) devs.push_back(d);
    } catch (...) {
        return AESW_ERR_NOMEM;
    }
    for (int d : devs)
        if (d < 0 || d >= n_dev) return AESW_ERR_NO_DEVICE;
    aesw_ctx *g = new (std::nothrow) aesw_ctx;
    if (!g) return AESW_ERR_NOMEM;
    try {
        g->members.reserve(devs.size());
    } catch (...) {
        delete g;
        return AESW_ERR_NOMEM;
    }
    for (int d : devs) {
        aesw_ctx *m = nullptr;
        const int rc = aesw_create(&m, d, sbox, mul2, mul3);
        if (rc != AESW_OK) {
            aesw_group_destroy(g);
            return rc;
        }
        m->group_size = (int)devs.size();
        g->members.push_back(m);  // (reserved above: cannot throw)
    }
    g->device = devs[0];
    *out = g;
    return AESW_OK;
}

int aesw_group_size(const aesw_ctx *ctx) { return ctx ? (int)ctx->members.size() : 0; }

aesw_ctx *aesw_group_member(aesw_ctx *ctx, uint32_t i) {
    return ctx && i < ctx->members.size() ? ctx->members[i] : nullptr;
}

}  // extern "C"
