// aesw_internal.h -- kernel parameter blocks and launchers shared by
// aesw_kernels.hip and the host code that launches them (aesw_api.cpp,
// aesw_hostpath.cpp; not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/aesw.h"
#include "aesw_check.h"
#include "aesw_placement.h"

namespace aesw {

struct KeyOut {
    uint8_t *w, *kx, *ky, *kz;  // any may be null
};

struct EncParams {
    const uint8_t *pt;      // n*16
    const uint8_t *keys;    // 16 or n*16; null when rk is used
    const uint32_t *rk;     // 44 words of a key scheduled earlier (aesw_schedule_key_device), or null
    const uint8_t *tables;  // 768: sbox | mul2 | mul3
    const uint32_t *ftab;   // flush descriptors of the layout (build_flush_tables), flush_table_words(layout) words
    uint8_t *x, *y, *z;     // column buffers (16-byte aligned)
    uint8_t *ct;            // n*16 or null
    KeyOut key;             // per-block-key mode only
    uint64_t n;
    uint32_t ngroups;       // block groups (16*waves blocks each); a workgroup strides over them
    uint32_t xcd_remap;     // xcd_group() mode: 0 dispatch order, 1 one contiguous eighth per XCD, C >= 2 turns of C groups
#ifdef AESW_TRACE
    uint64_t *trace;        // tools/trace.py only: 8 x u64 per wave
#endif
};

struct KeyParams {
    const uint8_t *keys;  // n*16
    const uint8_t *tables;
    KeyOut key;
    uint8_t *rk;  // n*176 or null
    uint64_t n;
    uint32_t ngroups;    // filled by the launcher
    uint32_t xcd_remap;  // xcd_group() mode, as in EncParams
};

// key mode: 0 = per-block keys, 1 = shared key expanded in the kernel, 2 = shared key scheduled earlier (p.rk)
hipError_t launch_encrypt(const EncParams &p, int layout, bool xt, int keymode, bool kemit, int waves, int store_mode,
                          uint32_t max_groups_in_flight, uint32_t xcd_remap, uint32_t lds_pad, hipStream_t s);
// flush-descriptor table of a layout (aesw_flush.h "scheduled flush"): size in 32-bit words, and the host-side builder
int flush_table_words(int layout);
void build_flush_tables(int layout, uint32_t *out);
// hipFuncSetAttribute(max dynamic LDS) for every instantiation, once per device: called by aesw_create()
hipError_t warm_launch_attributes();
hipError_t launch_key(const KeyParams &p, int layout, bool xt, int waves, int store_mode, uint32_t xcd_remap, hipStream_t s);
hipError_t launch_table(const uint8_t *tables, uint8_t *t0, uint8_t *t1, uint8_t *t2, uint8_t *t3, hipStream_t s);
struct AssembleParams {
    const uint8_t *x, *y, *z;        // n_blocks slabs
    const uint8_t *kw, *kx, *ky, *kz;  // one key slab (any may be null)
    const void *fr_lut;              // 256 x 32 B
    uint8_t *out;
    uint64_t n_blocks;
    uint32_t k, n_sets;
    uint32_t col_first, col_count;       // the advice columns to write (out holds col_count columns)
    uint32_t sx, sy, sz, kxs, kys, kzs;  // bytes per block / per key
    int packed;
    int geometry;         // Fr cells: 1 = one-shot 4 KiB workgroups on a (chunk, segment, column) grid, 0 = striding workgroups
    Placement place;      // blocks per column set (aesw_placement.h): filled by the launcher
};
static_assert(sizeof(AssembleParams) == 144 && offsetof(AssembleParams, n_blocks) == 72 && offsetof(AssembleParams, geometry) == 124 &&
              offsetof(AssembleParams, place) == 128 && offsetof(Placement, capn) == 8, "kernel arguments are read by offset");
hipError_t launch_assemble(const AssembleParams &p, bool as_fr, int store_mode, hipStream_t s);
// placement probe of aesw_columns_alloc: columns x, y, z, w, kx, ky, kz (null = absent) of n blocks
struct ProbeParams {
    uint8_t *col[7];
    uint32_t stride[7];
    uint32_t chunks[7];  // 4 KiB chunks per column (filled by the launcher for the linear fill)
    uint64_t n;
    uint32_t xcd_mode;  // xcd_group() mode of the context
};
hipError_t launch_probe(const ProbeParams &p, bool fill, hipStream_t s);
// aesw_check_witness_device (aesw_check.h): constraint satisfaction of n block slabs and their key slab(s)
struct CheckParams {
    const uint8_t *pt;          // n*16
    const uint8_t *keys;        // null, 16 (one key) or n*16
    const uint8_t *x, *y, *z;   // block columns in `layout` (DENSE or PACKED)
    const uint8_t *ct;          // n*16 or null
    const uint8_t *kw, *kx, *ky, *kz;  // one key slab, or n with per_block_keys
    const uint32_t *table;      // build_check_table(layout): CHK_WORDS words
    const uint8_t *tab768;      // sbox | mul2 | mul3
    uint64_t *report;           // aesw_check_report as 7 x u64
    uint64_t n;
    uint32_t per_block_keys;
    uint32_t skip_shared_key;   // one key slab for the batch: do not check it in this launch (a later chunk of a host-pointer call)
    uint32_t sx, sy, sz, kxs, kys, kzs, bi, img;  // strides, block image bytes, bytes of one wave's image region
};
inline void set_key_slab(CheckParams &p, const aesw_key_slab *ks) { p.kw = ks->w; p.kx = ks->kx; p.ky = ks->ky; p.kz = ks->kz; }
hipError_t launch_check(const CheckParams &p, hipStream_t s);
// The launch geometry of the three checker kernels (check_kernel, circ_check_kernel, cols_check_kernel): four waves per
// workgroup, one unit per wave at a time, and at most three workgroups (twelve waves) for each of the 256 CUs -- every wave
// strides over its share of the units.
constexpr uint32_t CHECK_WAVES = 4;
inline uint64_t check_groups(uint64_t units) {
    const uint64_t groups = (units + CHECK_WAVES - 1) / CHECK_WAVES;
    return groups < 256 * 3 ? groups : 256 * 3;
}
// Dynamic LDS of the part every checker kernel lays out first: fast table | tab768 | one image of `img` bytes per wave
// (ChkLayout<LAYOUT>::IMG).  What a kernel keeps behind it is its launcher's to add.
inline size_t check_lds_bytes(size_t img) { return (size_t)CHK_WORDS * 4 + 768 + CHECK_WAVES * img; }
hipError_t launch_expand_fr(const uint8_t *cells, uint64_t n_cells, const void *fr_lut, void *out, int store_mode, int geometry, hipStream_t s);

}  // namespace aesw

// Many circuits per launch (aesw_kernels.hip, namespace aesw_circ): circuit c owns blocks [offsets[c], offsets[c+1]).
namespace aesw_circ {
struct CircAsmParams {
    const uint8_t *x, *y, *z;          // the batch's block slabs
    const uint8_t *kw, *kx, *ky, *kz;  // n_circuits key slabs (any may be null)
    const void *fr_lut;
    uint8_t *out;                      // n_circuits x (3 n_sets + 1) << k cells
    const uint64_t *offsets;           // n_circuits + 1 (device)
    aesw::Placement place;             // filled by the launcher, as is cap = place.total(n_sets)
    uint64_t cap;
    uint32_t k, n_sets;
    uint32_t sx, sy, sz, kxs, kys, kzs;
    int packed;
    uint32_t c_first, cshift;          // filled by the launcher
};
static_assert(sizeof(CircAsmParams) == 152 && offsetof(CircAsmParams, offsets) == 72 && offsetof(CircAsmParams, place) == 80 &&
              offsetof(CircAsmParams, cap) == 96 && offsetof(CircAsmParams, k) == 104 && offsetof(CircAsmParams, cshift) == 144, "kernel arguments are read by offset");
hipError_t launch_assemble_circuits(const CircAsmParams &p, uint32_t n_circuits, bool as_fr, hipStream_t s);
}  // namespace aesw_circ

