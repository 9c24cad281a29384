// aesw_ctx.h -- the opaque context of include/aesw.h and the small helpers every translation unit of the C ABI uses
// (aesw_api.cpp: context, options and the device-pointer entry points; aesw_keyring.cpp: the scheduled key's round-key slots;
// aesw_hostpath.cpp: the host-pointer entry points and their two-stage pipeline; aesw_arena.cpp: the probed column arena;
// aesw_group.cpp: device groups; aesw_circuits.cpp: many circuits per launch), and the few internal functions one of them takes from
// another.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/aesw.h"
#include "aesw_align.h"
#include "aesw_keyring.h"
#include "aesw_options.h"

struct aesw_ctx {
    int device = -1;
    uint8_t *d_tables = nullptr;  // 768 B
    uint8_t *d_fr_lut = nullptr;  // 256 x 32 B
    uint32_t *d_ftab[3] = {nullptr, nullptr, nullptr};  // flush descriptors per layout (aesw_flush.h "scheduled flush")
    uint32_t *d_chktab[2] = {nullptr, nullptr};         // check tables of the DENSE / PACKED layout (aesw_check.h), uploaded by aesw_create
    KeyRing keys;  // the scheduled key: its round-key slots and their ordering (aesw_keyring.h)
    bool xt = false;
    AeswOptions opt;  // every knob aesw_set_option stores (aesw_options.h)
    double best_fill_us_per_gb = 0;  // fastest linear fill any arena search of this context has seen (us per 10^9 bytes): the probe's yardstick
    struct ArenaRange { void *p; size_t bytes; bool vmm; };  // vmm: built with the virtual-memory API (freed by unmap), else hipMalloc
    // A probed arena: its ranges, and what it was placed for (the shape decides whether a later request may take it over)
    struct ArenaRec {
        void *key;
        std::vector<ArenaRange> ranges;
        uint64_t n = 0;
        int layout = 0, with_key_slab = 0, with_ct = 0;
        uint32_t xcd = 0;          // the "xcd_remap" the store pattern was probed with
        aesw_columns cols = {};    // the column pointers and probe results handed to the caller
        uint64_t stamp = 0;        // when it was freed (cache order)
    };
    std::vector<ArenaRec> vmm_arenas;  // arenas built with the virtual-memory API (one range per column; freed by unmap, not hipFree)
    // Placement cache: a probed arena that is freed keeps its backing (physical placement is what the search paid for); the next
    // aesw_columns_alloc of the same shape takes it over without a search.  Bounded by option "arena_cache_max_mb", oldest out first;
    // flushed when a search runs short of memory, by option "arena_cache" = 0 and by aesw_destroy.
    std::vector<ArenaRec> arena_cache;
    uint64_t arena_stamp = 0;
    uint64_t arena_cache_hits = 0;
#ifdef AESW_TRACE
    uint64_t *trace = nullptr;
#endif
    std::string last_error;
    hipStream_t s_compute = nullptr, s_copy = nullptr;
    hipStream_t s_batch[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint8_t *bounce[2] = {nullptr, nullptr};  // page-locked staging for pageable destinations
    size_t bounce_bytes = 0;
    uint8_t *scratch = nullptr;  // device buffers of the host-pointer path (grow-only)
    size_t scratch_bytes = 0;
    aesw_stream_stats stats = {};  // of the last streaming call
    aesw_check_report stream_report = {0, 0, 0, 0, 0, 0, ~0ull};  // of the last streaming call with "stream_check" on
    // Group context (aesw_create_group, aesw_group.cpp): one member context per listed device, nothing on a device of its own; the
    // host-pointer entry points split a batch into block shards over the members.  Empty for a plain context.
    std::vector<aesw_ctx *> members;
    int group_size = 1;  // of a MEMBER: the members of its group (its automatic "copy_threads" is its share of the CPUs)
};

// aesw_group.cpp: what the entry points of aesw_api.cpp and aesw_hostpath.cpp hand a group context to (a short branch at their top)
inline bool aesw_is_group(const aesw_ctx *ctx) { return ctx && !ctx->members.empty(); }
int aesw_group_refuse(aesw_ctx *group, const char *entry);  // AESW_ERR_INVALID_ARG: device pointers belong to one GPU
void aesw_group_destroy(aesw_ctx *group);
int aesw_group_set_option(aesw_ctx *group, const char *name, int64_t value);
int aesw_group_encrypt_witness(aesw_ctx *group, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout,
                               uint8_t *x, uint8_t *y, uint8_t *z, uint8_t *ct, const aesw_key_slab *ks);
int aesw_group_encrypt_witness_stream(aesw_ctx *group, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout,
                                      aesw_chunk_fn consume, void *user);
int aesw_group_key_schedule_witness(aesw_ctx *group, const uint8_t *keys, uint64_t n, int layout, uint8_t *w, uint8_t *kx, uint8_t *ky,
                                    uint8_t *kz, uint8_t *rk);
int aesw_group_check_witness(aesw_ctx *group, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, int layout,
                             const uint8_t *x, const uint8_t *y, const uint8_t *z, const uint8_t *ct, const aesw_key_slab *ks,
                             aesw_check_report *report);
int aesw_group_schedule_key(aesw_ctx *group, const uint8_t key[16], int layout, const aesw_key_slab *ks);
int aesw_group_lookup_table(aesw_ctx *group, uint8_t *t0, uint8_t *t1, uint8_t *t2, uint8_t *t3);

inline int fail_hip(aesw_ctx *ctx, hipError_t e, const char *what) {
    if (ctx) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        ctx->last_error = buf;
    }
    return e == hipErrorOutOfMemory ? AESW_ERR_NOMEM : AESW_ERR_HIP;
}

#define HIP_TRY(ctx, expr)                                  \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return fail_hip(ctx, e_, #expr); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

void aesw_arena_cache_trim(aesw_ctx *ctx, uint64_t keep_bytes);  // aesw_arena.cpp: release cached arenas, oldest first, until keep_bytes stay

// a key slab a checker library reads 16 bytes at a time: all four columns there and 16-byte aligned
inline bool key_slab_ok(const aesw_key_slab *ks) {
    return ks && ks->w && ks->kx && ks->ky && ks->kz && aligned_to(ks->w, 16) && aligned_to(ks->kx, 16) && aligned_to(ks->ky, 16) && aligned_to(ks->kz, 16);
}
inline uint64_t now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// Fold the report of one part of a batch (a pipeline stage, a group member's shard) into the batch-wide one.  Units of a part count
// from its first block -- a block, or a per-block key slab; the one slab of a shared key is unit 0 of the batch as well.
inline void merge_check_report(aesw_check_report &t, const aesw_check_report &r, uint64_t first_block, bool per_block_keys) {
    t.blocks += r.blocks; t.keys += r.keys;
    t.lookup_failures += r.lookup_failures; t.copy_failures += r.copy_failures;
    t.gate_failures += r.gate_failures; t.input_failures += r.input_failures;
    if (r.first == AESW_CHECK_NONE) return;
    const uint64_t unit = AESW_CHECK_UNIT(r.first) + ((!per_block_keys && AESW_CHECK_IS_KEY_SLAB(r.first)) ? 0 : first_block);
    const uint64_t f = unit << 20 | (r.first & 0xfffffu);
    if (f < t.first) t.first = f;
}

inline bool aesw_valid_layout(int l) { return l == AESW_LAYOUT_DENSE || l == AESW_LAYOUT_PACKED || l == AESW_LAYOUT_VALUES; }

// What aesw_hostpath.cpp takes from aesw_api.cpp, and the one thing aesw_get_option takes back (AESW_INTERNAL: aesw_keyring.h).
namespace aesw { struct AssembleParams; }
// the argument checks of the assemble entry points and the launch parameters of all 3 n_sets + 1 columns
AESW_INTERNAL int fill_assemble_params(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x,
                                       const uint8_t *d_y, const uint8_t *d_z, const aesw_key_slab *ks, aesw::AssembleParams *p);
// aesw_check_witness_device, optionally without the shared key slab (a later chunk of a host-pointer call)
AESW_INTERNAL int check_witness_impl(aesw_ctx *ctx, const uint8_t *d_pt, const uint8_t *d_keys, int per_block_keys, uint64_t n, int layout,
                                     const uint8_t *d_x, const uint8_t *d_y, const uint8_t *d_z, const uint8_t *d_ct, const aesw_key_slab *ks,
                                     aesw_check_report *d_report, void *stream, bool skip_shared_key);
AESW_INTERNAL int auto_copy_threads(const aesw_ctx *ctx);  // aesw_hostpath.cpp: what "copy_threads" resolves to ("effective_copy_threads")
