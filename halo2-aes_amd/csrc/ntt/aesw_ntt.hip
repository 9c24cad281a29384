// ntt/aesw_ntt.hip -- libaesw_ntt.so (include/aesw_ntt.h): columns of Fr cells between Lagrange, coefficient and extended-coset form
// (DESIGN.md 4.22).  The field is aesw_fr.h's and the rules -- the pass plan, which cell sits in which slot of which workgroup, the
// twiddle of a load and of a butterfly, the LDS swizzle, the tables, the workspace -- are aesw_ntt.h's; nothing of either is
// restated here.  What is here:
//   * ntt_tables_kernel: a thread raises a root to one power;
//   * ntt_pass_kernel<NT>: a workgroup loads its tile of 2^NTT_PASS_LOG cells of one column (grid.y) into LDS, limb-planar -- the
//     first pass bit-reversed, zero behind the input's rows and times the zeta cycle where the call asks for it, a later pass times
//     the four-step twiddle --, runs the pass's stages with a barrier behind each, and writes the tile back; the last pass
//     multiplies by 1/2^k and the inverse zeta cycle where the call asks for it and stores through aesw_store.h's flavour;
//   * the four entry points over one launcher, and the checks that are theirs alone.
// No atomic, no look-back flag, nothing to reset: the passes are ordered by the stream and every output word is stored once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_ntt.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_ntt.h"

namespace aesw_ntt {
using namespace aesw;

constexpr uint32_t THREADS = NTT_THREADS;
static_assert(sizeof(Fr) == 32, "a cell is two 16-byte pieces");

// Which passes a transform enqueues: all of them, except in a measurement variant built with -DAESW_NTT_PASSES=<mask>
// (tests/test_perf_ntt.py prices one pass at a time that way; such a library's outputs are of no use).
#ifndef AESW_NTT_PASSES
#define AESW_NTT_PASSES 0xffffffffu
#endif
constexpr uint32_t PASSES = AESW_NTT_PASSES;

typedef uint32_t Tile[FR_LIMBS][NTT_SLOTS];  // limb-planar (aesw_ntt.h, ntt_lds_index)
__device__ __forceinline__ Fr tile_read(const Tile &tile, uint32_t slot) {
    const uint32_t at = ntt_lds_index(slot);
    Fr v = FR_ZERO;
#pragma unroll
    for (int i = 0; i < FR_LIMBS; ++i) v.l[i] = tile[i][at];
    return v;
}
__device__ __forceinline__ void tile_write(Tile &tile, uint32_t slot, const Fr &v) {
    const uint32_t at = ntt_lds_index(slot);
#pragma unroll
    for (int i = 0; i < FR_LIMBS; ++i) tile[i][at] = v.l[i];
}

// ---- the tables -------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(THREADS) ntt_tables_kernel(u32x4 *out, uint32_t max_k, uint32_t cells) {
    const uint32_t at = blockIdx.x * THREADS + threadIdx.x;
    if (at < cells) store_cell<0>(cell_at(out, at), ntt_table_cell(max_k, at));
}

// ---- a pass -----------------------------------------------------------------------------------------------------------------

enum : uint32_t {
    F_INVERSE = 1,     // the roots are the inverses
    F_FIRST = 2,       // the bit-reversed load from the call's input
    F_ZETA_LOAD = 4,   // ... times zeta^(i mod 3)
    F_SCALE = 8,       // the store times 1/2^k
    F_ZETA_STORE = 16  // ... and zeta^-(i mod 3)
};

struct PassParams {
    const u32x4 *src;  // [n_cols][2^src_k]
    u32x4 *dst;        // [n_cols][2^k]; may be src: a workgroup reads its cells before it writes them, and no other's
    const u32x4 *short_t, *low, *high, *scales;
    uint32_t k, src_k, max_k, zeta_sel, flags;
    NttPass pass;
};

// omega_(2^max_k) to an exponent below 2^max_k: two cells and a product (4.21's split)
__device__ __forceinline__ Fr root_power(const PassParams &p, uint32_t e) {
    return fr_mul(load_cell(cell_at(p.low, ntt_low_index(e))), load_cell(cell_at(p.high, ntt_high_index(e))));
}

// grid: x = the tile, y = the column
template <int NT>
__global__ void __launch_bounds__(THREADS) ntt_pass_kernel(const PassParams p) {
    __shared__ Tile tile;
    const uint32_t w = blockIdx.x;
    const NttPass q = p.pass;
    const bool inverse = p.flags & F_INVERSE;
    const u32x4 *src = cell_at(p.src, (uint64_t)blockIdx.y << p.src_k);
    u32x4 *dst = cell_at(p.dst, (uint64_t)blockIdx.y << p.k);

#pragma unroll 1
    for (uint32_t slot = threadIdx.x; slot < NTT_SLOTS; slot += THREADS) {
        const uint32_t position = ntt_slot_position(q, w, slot);
        Fr v = FR_ZERO;
        if (p.flags & F_FIRST) {
            const uint32_t i = ntt_first_source(p.k, position);
            if (i >> p.src_k == 0) {  // behind the input's rows: zero padding
                v = load_cell(cell_at(src, i));
                if (p.flags & F_ZETA_LOAD) {
                    const uint32_t e = ntt_zeta_exponent(p.zeta_sel, i, false);
                    if (e) v = fr_mul(v, load_cell(cell_at(p.scales, ntt_scale_index(0, e))));
                }
            }
        } else {
            const uint32_t e = ntt_slot_twiddle(q, w, slot);
            v = fr_mul(load_cell(cell_at(src, position)), root_power(p, ntt_root_exponent(p.max_k, q.s0 + q.m, e, inverse)));
        }
        tile_write(tile, slot, v);
    }
    __syncthreads();

#pragma unroll 1
    for (uint32_t j = 1; j <= q.m; ++j) {
        const uint32_t span = ntt_butterfly_span(q, j);
#pragma unroll 1
        for (uint32_t b = threadIdx.x; b < NTT_SLOTS / 2; b += THREADS) {
            const uint32_t lower = ntt_butterfly_slot(q, j, b);
            const Fr x = tile_read(tile, lower);
            Fr y = tile_read(tile, lower + span);
            if (j > 1) y = fr_mul(y, load_cell(cell_at(p.short_t, ntt_butterfly_twiddle(q, j, lower, inverse))));  // stage 1 multiplies by 1
            tile_write(tile, lower, fr_add(x, y));
            tile_write(tile, lower + span, fr_sub(x, y));
        }
        __syncthreads();
    }

#pragma unroll 1
    for (uint32_t slot = threadIdx.x; slot < NTT_SLOTS; slot += THREADS) {
        const uint32_t position = ntt_slot_position(q, w, slot);
        Fr v = tile_read(tile, slot);
        if (p.flags & F_SCALE) {
            const uint32_t e = p.flags & F_ZETA_STORE ? ntt_zeta_exponent(p.zeta_sel, position, true) : 0u;
            v = fr_mul(v, load_cell(cell_at(p.scales, ntt_scale_index(p.k, e))));
        }
        store_cell<NT>(cell_at(dst, position), v);
    }
}

// ---- the launcher ---------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

struct Call {
    const char *name;
    uint32_t k, src_k, zeta_sel, n_cols, max_k;
    uint32_t first, last;  // flags of the first and of the last pass, F_INVERSE for all
    bool in_place_allowed;
};

// what the four calls check alike, in this order; then the passes
static int transform(aesw_ctx *ctx, const Call &c, const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_tables, void *d_workspace, void *stream) {
    if (int rc = entry_refused(ctx, c.name)) return rc;
    if (!ntt_k_ok(c.src_k) || !ntt_k_ok(c.k) || c.src_k > c.k) return refuse(ctx, c.name, "k (and ext_k, no smaller) must be 10 ... 28 (the field's 2-adicity is 28)");
    if (!ntt_k_ok(c.max_k) || c.k > c.max_k) return refuse(ctx, c.name, "max_k must be 10 ... 28 and no smaller than the transform's k");
    if (!ntt_cols_ok(c.n_cols)) return refuse(ctx, c.name, "n_cols must be 1 ... 65535");
    if (c.zeta_sel > 1) return refuse(ctx, c.name, "zeta_sel must be 0 or 1");
    if (!d_in || !d_out || !aligned_to(d_in, 16) || !aligned_to(d_out, 16)) return refuse(ctx, c.name, "the input and the output must be there and 16-byte aligned");
    if (!d_tables || !aligned_to(d_tables, 16)) return refuse(ctx, c.name, "d_tables must be there and 16-byte aligned");
    const uint64_t in_bytes = ntt_cells(c.src_k, c.n_cols) * sizeof(Fr), out_bytes = ntt_cells(c.k, c.n_cols) * sizeof(Fr);
    const bool in_place = d_in == d_out;
    if (in_place ? !c.in_place_allowed : overlap(d_in, in_bytes, d_out, out_bytes))
        return refuse(ctx, c.name, c.in_place_allowed ? "the input and the output must be one buffer or must not overlap" : "the input and the output must not overlap");
    if (overlap(d_tables, ntt_tables_bytes(c.max_k), d_out, out_bytes)) return refuse(ctx, c.name, "d_tables must not overlap the output");
    const uint32_t passes = ntt_passes(c.k);
    const bool needs_workspace = in_place && passes > 1;
    if (!aligned_to(d_workspace, 16) || (needs_workspace && !d_workspace))
        return refuse(ctx, c.name, "d_workspace must be 16-byte aligned, and there for an in-place call of more than one pass");
    if (needs_workspace && (overlap(d_workspace, out_bytes, d_out, out_bytes) || overlap(d_workspace, out_bytes, d_tables, ntt_tables_bytes(c.max_k))))
        return refuse(ctx, c.name, "d_workspace must not overlap the columns or the tables");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const NttTables t = ntt_tables(c.max_k);
    const u32x4 *tables = reinterpret_cast<const u32x4 *>(d_tables);
    PassParams p{};
    p.short_t = tables + (uint64_t)t.short_at * 2;
    p.low = tables + (uint64_t)t.low_at * 2;
    p.high = tables + (uint64_t)t.high_at * 2;
    p.scales = tables + (uint64_t)t.scales_at * 2;
    p.k = c.k; p.max_k = c.max_k; p.zeta_sel = c.zeta_sel;
    u32x4 *const out = reinterpret_cast<u32x4 *>(d_out), *const between = needs_workspace ? static_cast<u32x4 *>(d_workspace) : out;
    const dim3 grid(ntt_workgroups(c.k), c.n_cols);  // at most 2^27 tiles (a measurement build), 65535 columns
    for (uint32_t i = 0; i < passes; ++i) {
        const bool first = i == 0, last = i + 1 == passes;
        p.pass = ntt_pass(c.k, i);
        p.src = first ? reinterpret_cast<const u32x4 *>(d_in) : between;
        p.src_k = first ? c.src_k : c.k;
        p.dst = last ? out : between;
        p.flags = (c.first & F_INVERSE) | (first ? c.first | F_FIRST : 0u) | (last ? c.last : 0u);
        if (!(PASSES >> i & 1u)) continue;
        if (last) with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(ntt_pass_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, p); });
        else hipLaunchKernelGGL(ntt_pass_kernel<0>, grid, dim3(THREADS), 0, s, p);
        HIP_TRY(ctx, hipGetLastError());
    }
    return AESW_OK;
}

}  // namespace aesw_ntt

extern "C" {

size_t aesw_ntt_tables_bytes(uint32_t max_k) { return (size_t)aesw::ntt_tables_bytes(max_k); }
size_t aesw_ntt_workspace_bytes(uint32_t k, uint32_t n_cols) { return (size_t)aesw::ntt_workspace_bytes(k, n_cols); }

int aesw_ntt_tables_device(aesw_ctx *ctx, uint32_t max_k, uint8_t *d_tables, void *stream) {
    using namespace aesw_ntt;
    const char *const call = "aesw_ntt_tables_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!ntt_k_ok(max_k)) return refuse(ctx, call, "max_k must be 10 ... 28 (the field's 2-adicity is 28)");
    if (!d_tables || !aligned_to(d_tables, 16)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const uint32_t cells = ntt_tables(max_k).cells;  // at most 2^15 + 2^10 + 87
    hipLaunchKernelGGL(ntt_tables_kernel, dim3((cells + THREADS - 1) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<u32x4 *>(d_tables), max_k, cells);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_ntt_lagrange_to_coeff_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_tables, uint32_t max_k,
                                      void *d_workspace, void *stream) {
    using namespace aesw_ntt;
    return transform(ctx, Call{"aesw_ntt_lagrange_to_coeff_device", k, k, 0, n_cols, max_k, F_INVERSE, F_SCALE, true}, d_in, d_out, d_tables, d_workspace, stream);
}

int aesw_ntt_coeff_to_lagrange_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint8_t *d_in, uint8_t *d_out, const uint8_t *d_tables, uint32_t max_k,
                                      void *d_workspace, void *stream) {
    using namespace aesw_ntt;
    return transform(ctx, Call{"aesw_ntt_coeff_to_lagrange_device", k, k, 0, n_cols, max_k, 0, 0, true}, d_in, d_out, d_tables, d_workspace, stream);
}

int aesw_ntt_coeff_to_extended_device(aesw_ctx *ctx, uint32_t k, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_cols, const uint8_t *d_coeff, uint8_t *d_ext,
                                      const uint8_t *d_tables, uint32_t max_k, void *d_workspace, void *stream) {
    using namespace aesw_ntt;
    return transform(ctx, Call{"aesw_ntt_coeff_to_extended_device", ext_k, k, zeta_sel, n_cols, max_k, F_ZETA_LOAD, 0, false}, d_coeff, d_ext, d_tables, d_workspace,
                     stream);
}

int aesw_ntt_extended_to_coeff_device(aesw_ctx *ctx, uint32_t ext_k, uint32_t zeta_sel, uint32_t n_cols, const uint8_t *d_ext, uint8_t *d_coeff,
                                      const uint8_t *d_tables, uint32_t max_k, void *d_workspace, void *stream) {
    using namespace aesw_ntt;
    return transform(ctx, Call{"aesw_ntt_extended_to_coeff_device", ext_k, ext_k, zeta_sel, n_cols, max_k, F_INVERSE, F_SCALE | F_ZETA_STORE, true}, d_ext, d_coeff,
                     d_tables, d_workspace, stream);
}

}  // extern "C"
