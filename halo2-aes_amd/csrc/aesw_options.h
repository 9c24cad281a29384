// aesw_options.h -- the options of aesw_set_option / aesw_get_option, described once: the knobs they are stored in (AeswOptions,
// embedded in aesw_ctx as `opt`) and one table row per name (AESW_OPTIONS): the field, what values it accepts, whether it can be
// set and read, and whether aesw_api.cpp has something to add that a row cannot say.  The prose for users is the comment in front
// of aesw_set_option in include/aesw.h.  No HIP call and no ROCm include: tests/test_option_table.py compiles this header alone
// with g++ and holds every row against the values the library has always accepted.  Not part of the public ABI.
#pragma once
#include <cstdint>
#include <cstring>

// Every knob is an int64_t, the type the two entry points carry: a row names its field with one pointer-to-member.  Where a use
// narrows one (a store flavour to int, "xcd_remap" to uint32_t, a shift count) it is the row's range that keeps the value in the narrower type.
struct AeswOptions {
    int64_t waves_shared = 0;  // waves per group, shared-key kernels (0 = auto)
    int64_t waves_pbk = 0;     // per-block-key and key kernels (0 = auto)
    int64_t nt = 1;  // store flavour: 0 plain, 1 nontemporal (default since round 3), 2 write-through (sc1).  With all three flavours compiled to the
                     // same code (round 3: they used to differ by 60 VGPRs, i.e. in residency) nontemporal stores are 1-3 % ahead at 2^20 blocks on
                     // well-placed columns and within +-2 % of sc1 elsewhere (profiles/r03_study/README.md)
    int64_t key_nt = 1;  // store flavour of key_kernel (one contiguous flush per column at the end): nontemporal 4-9 % ahead of sc1 (tools/keysweep.py)
    int64_t fr_geo = 1;  // geometry of expand_fr: 1 = one-shot 4 KiB workgroups, LUT gathered from global memory: 7.3 TB/s with nontemporal stores
                         // against 5.2 for 0 = striding workgroups + LDS LUT and 5.9 for 2 = one-shot 16 KiB + LDS LUT (tools/frsweep.py)
    int64_t asm_geo = 4;  // geometry of the Fr form of assemble: 0 striding workgroups, 1 one-shot (chunk, segment, column) grid, 2 / 3 / 4 one-shot workgroups
                          // on aligned output chunks: 256 threads x 1 piece, 256 x 2, 128 x 2 (4 = default: 6.9 TB/s for K = 20, N = 5 against 5.3 striding)
                          // workgroups on a (chunk, segment, column) grid (round 3: byte-exact, 5.2 TB/s -- a piece is a chain of three dependent loads
                          // (index table, slab byte, LUT) and a one-shot workgroup has nothing else in flight: latency x residency bounds it, not divisions)
    int64_t fr_nt = 1;  // store flavour of the Fr-expanding kernels: nontemporal measured 19 % ahead of plain and sc1 there (tools/frsweep.py)
    int64_t grid_cap = 0;  // max workgroups per launch (0 = one per block group)
    int64_t xcd_remap = 1;  // xcd_group() mode: 0 dispatch order, 1 one contiguous eighth of the groups per XCD (+3-4 % at 2^20 blocks over 0, tools/sweep.py xcd), C >= 2 turns of C groups
    int64_t lds_pad = 0;  // diagnostic (tools/occ.py): extra dynamic LDS per workgroup, lowers residency
    int64_t arena_align_log2 = 0;  // aesw_columns_alloc: column alignment (0 = auto: 2 MiB)
    int64_t arena_probe = -1;      // candidate backings aesw_columns_alloc measures per unit (-1 = auto, 0 = none: one hipMalloc)
    int64_t arena_unit = 2;        // what a candidate is: 0 = the whole set of columns in one range, 1 = one column (greedy, largest first),
                                   // 2 = whole sets first, columns if no set candidate runs the pattern as fast as its fill (default)
    int64_t arena_cache_on = 1;    // the placement cache of aesw_ctx::arena_cache is in use
    int64_t arena_cache_max_mb = 65536;  // ... and may hold this much (MiB), oldest out first
    int64_t arena_probe_budget_ms = 3000;  // a search stops building candidates once it has run this long (0 = no limit); it always keeps the best so far
    int64_t chunk_blocks = 1 << 15;  // host-pointer path: blocks per pipeline stage
    int64_t copy_threads = -1;       // host threads that move a stage from the page-locked bounce buffer into a pageable destination (-1 = auto)
    int64_t split_small = 0;    // experiment of round 4 (profiles/r04_study/split_small.md): a LONE shared / scheduled-key launch of 2^15 .. 2^17 blocks
                                // dealt as this many line-aligned sub-ranges onto the internal streams (0 / 1 = off)
    int64_t batch_streams = 3;  // aesw_encrypt_witness_batches_device: internal streams the batches are dealt onto
    int64_t stream_check = 0;   // aesw_encrypt_witness_stream checks every chunk on the device before it travels (aesw_check.h)
    int64_t stream_poison = 0;  // diagnostic (tests): block index + 1 whose y / z cells the stream overwrites before its chunk is checked and shipped
    uint64_t arena_cache_max_bytes() const { return (uint64_t)arena_cache_max_mb << 20; }
};

enum : uint8_t {
    OPT_SET = 1, OPT_GET = 2, OPT_RW = 3, OPT_OR_ZERO = 4,  // aesw_set_option / aesw_get_option take the name; 0 is accepted besides lo ... hi
    OPT_TRUTHY = 8,      // any value is accepted; stores value != 0 and reads field == 1 ("nt_stores", the older name of "store_mode" 0 / 1)
    OPT_TRACE_ONLY = 16  // settable in a -DAESW_TRACE build of the library only (an unknown name to any other), and not in the prose of aesw.h
};
// What aesw_api.cpp adds to a row: a follow-up behind a set, or the value of a get that is in no field of AeswOptions.
enum class OptExtra : uint8_t {
    NONE, ARENA_CACHE, ARENA_CACHE_MAX_MB,  // set: release what is cached now (0) / trim the cache to the new bound
    KEY_SLOTS, FORCE_TABLE_PATH, TRACE_PTR,  // in the key ring / one way: 1 clears aesw_ctx::xt, reads !xt / aesw_ctx::trace
    EFFECTIVE_WAVES_SHARED, EFFECTIVE_WAVES_PBK, EFFECTIVE_WAVES_KEY, EFFECTIVE_COPY_THREADS,  // what a launch really uses
    ARENA_CACHE_HITS, ARENA_CACHED_BYTES, KEY_READER_WAITS, KEY_WRITER_WAITS, KEY_SLOTS_ALLOCATED, KEY_SLOTS_PINNED,  // statistics
};
struct OptionRow {
    const char *name;
    int64_t AeswOptions::*field;  // null: the value is not in AeswOptions (`extra` says where it is)
    int64_t lo, hi;               // accepted values, stored as they are (a boolean is 0 ... 1)
    uint8_t access;               // OPT_* flags
    OptExtra extra = OptExtra::NONE;
};
#ifdef AESW_DIAGNOSTIC
constexpr int64_t OPT_STORE_MODE_MAX = 5;  // 3 ... 5: "leave the flush out" and its kin (output is garbage), tools/ only
#else
constexpr int64_t OPT_STORE_MODE_MAX = 2;
#endif
inline constexpr OptionRow AESW_OPTIONS[] = {
    // name                    field                                lo         hi                  access (, extra)
    {"waves_shared",           &AeswOptions::waves_shared,          0,         4,                  OPT_RW},
    {"waves_pbk",              &AeswOptions::waves_pbk,             0,         4,                  OPT_RW},
    {"nt_stores",              &AeswOptions::nt,                    INT64_MIN, INT64_MAX,          OPT_RW | OPT_TRUTHY},
    {"store_mode",             &AeswOptions::nt,                    0,         OPT_STORE_MODE_MAX, OPT_RW},
    {"key_store_mode",         &AeswOptions::key_nt,                0,         2,                  OPT_RW},
    {"fr_geometry",            &AeswOptions::fr_geo,                0,         2,                  OPT_RW},
    {"fr_store_mode",          &AeswOptions::fr_nt,                 0,         2,                  OPT_RW},
    {"assemble_geometry",      &AeswOptions::asm_geo,               0,         4,                  OPT_RW},
    {"grid_cap",               &AeswOptions::grid_cap,              0,         0x7fffffff,         OPT_RW},
    {"xcd_remap",              &AeswOptions::xcd_remap,             0,         1 << 24,            OPT_RW},
    {"lds_pad",                &AeswOptions::lds_pad,               0,         120 * 1024,         OPT_RW},
    {"arena_align_log2",       &AeswOptions::arena_align_log2,      7,         32,                 OPT_RW | OPT_OR_ZERO},
    {"arena_probe",            &AeswOptions::arena_probe,           -1,        64,                 OPT_RW},
    {"arena_unit",             &AeswOptions::arena_unit,            0,         2,                  OPT_RW},
    {"trace_ptr",              nullptr,                             INT64_MIN, INT64_MAX,          OPT_SET | OPT_TRACE_ONLY, OptExtra::TRACE_PTR},
    {"force_table_path",       nullptr,                             INT64_MIN, INT64_MAX,          OPT_RW, OptExtra::FORCE_TABLE_PATH},
    {"chunk_blocks",           &AeswOptions::chunk_blocks,          64,        INT64_MAX,          OPT_RW},
    {"batch_streams",          &AeswOptions::batch_streams,         1,         8,                  OPT_RW},
    {"copy_threads",           &AeswOptions::copy_threads,          -1,        64,                 OPT_RW},
    {"key_slots",              nullptr,                             1,         64,                 OPT_RW, OptExtra::KEY_SLOTS},
    {"split_small",            &AeswOptions::split_small,           0,         8,                  OPT_RW},
    {"stream_check",           &AeswOptions::stream_check,          0,         1,                  OPT_RW},
    {"stream_poison",          &AeswOptions::stream_poison,         0,         INT64_MAX,          OPT_RW},
    {"arena_cache",            &AeswOptions::arena_cache_on,        0,         1,                  OPT_RW, OptExtra::ARENA_CACHE},
    {"arena_cache_max_mb",     &AeswOptions::arena_cache_max_mb,    0,         (int64_t)1 << 30,   OPT_RW, OptExtra::ARENA_CACHE_MAX_MB},
    {"arena_probe_budget_ms",  &AeswOptions::arena_probe_budget_ms, 0,         600000,             OPT_RW},
    // read only: what a launch really uses (0 = auto resolved, values above the layout's maximum clamped; packed layout), and statistics
    {"effective_waves_shared", nullptr,                             0,         0,                  OPT_GET, OptExtra::EFFECTIVE_WAVES_SHARED},
    {"effective_waves_pbk",    nullptr,                             0,         0,                  OPT_GET, OptExtra::EFFECTIVE_WAVES_PBK},
    {"effective_waves_key",    nullptr,                             0,         0,                  OPT_GET, OptExtra::EFFECTIVE_WAVES_KEY},
    {"effective_copy_threads", nullptr,                             0,         0,                  OPT_GET, OptExtra::EFFECTIVE_COPY_THREADS},
    {"arena_cache_hits",       nullptr,                             0,         0,                  OPT_GET, OptExtra::ARENA_CACHE_HITS},
    {"arena_cached_bytes",     nullptr,                             0,         0,                  OPT_GET, OptExtra::ARENA_CACHED_BYTES},
    {"key_reader_waits",       nullptr,                             0,         0,                  OPT_GET, OptExtra::KEY_READER_WAITS},
    {"key_writer_waits",       nullptr,                             0,         0,                  OPT_GET, OptExtra::KEY_WRITER_WAITS},
    {"key_slots_allocated",    nullptr,                             0,         0,                  OPT_GET, OptExtra::KEY_SLOTS_ALLOCATED},
    {"key_slots_pinned",       nullptr,                             0,         0,                  OPT_GET, OptExtra::KEY_SLOTS_PINNED},
};
inline const OptionRow *aesw_find_option(const char *name) {
    for (const OptionRow &r : AESW_OPTIONS) if (!std::strcmp(name, r.name)) return &r;
    return nullptr;
}
// The set of one row: false (and nothing stored) if the name cannot be set or refuses the value.  A row without a field stores
// nothing here: its OptExtra case in aesw_set_option does.
inline bool aesw_option_set(AeswOptions &o, const OptionRow &r, int64_t v) {
#ifndef AESW_TRACE
    if (r.access & OPT_TRACE_ONLY) return false;
#endif
    const bool truthy = r.access & OPT_TRUTHY, zero = (r.access & OPT_OR_ZERO) && v == 0;
    if (!(r.access & OPT_SET) || !(truthy || zero || (v >= r.lo && v <= r.hi))) return false;
    if (r.field) o.*r.field = truthy ? (v != 0 ? 1 : 0) : v;
    return true;
}
// The get of one row that has a field; false for a name that cannot be read and for a row without a field (its OptExtra case in
// aesw_get_option computes the value).
inline bool aesw_option_get(const AeswOptions &o, const OptionRow &r, int64_t *v) {
    if (!(r.access & OPT_GET) || !r.field) return false;
    *v = (r.access & OPT_TRUTHY) ? (o.*r.field == 1 ? 1 : 0) : o.*r.field;
    return true;
}
