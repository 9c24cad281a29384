// perm/aesw_perm.hip -- libaesw_perm.so (include/aesw_perm.h): plookup's permuted columns as columns of table-row indices, built
// from the lookup multiplicities, and the gather that turns such a column into Fr cells.  The rule -- the
// clipped sums, the workspace, the search, the leftover list, what stands at a position -- is aesw_perm.h's and the sections
// are aesw_mult.h's; nothing of either is restated here.  What is here:
//   * perm_scan_kernel: one workgroup per argument streams the argument's section in tiles of 4 096 bins -- four consecutive
//     bins per thread, a wave scan, the wave totals through LDS, the carry in a register -- twice per tile: the clipped sums,
//     then the rows they leave with a count.  It writes the argument's three arrays and four scalars to the workspace;
//   * perm_expand_kernel: driven by position.  A lane owns four consecutive positions of one argument: it searches the starts
//     for its first and its last position, the two between them inside that range, and stores 16 bytes of A' and 16 of S'.
//     One-shot workgroups of 4 KiB per column, in address order.  Workgroup (0, 0) also writes the report, from the overflow
//     flags of the workspace (the fold is aesw_report_dev.h's): plain stores, no atomic, nothing to reset;
//   * perm_gather_fr_kernel<NT>: expand_fr_kernel's one-shot geometry over the caller's 66 561-cell table, the store flavour
//     aesw_store.h's;
//   * the entry points and the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_perm.h"
#include "../aesw_entry.h"
#include "../aesw_perm.h"
#include "../aesw_report_dev.h"
#include "../aesw_store.h"

namespace aesw_perm {
using namespace aesw;

constexpr int SCAN_WAVES = 16, SCAN_THREADS = SCAN_WAVES * LANES, PER_THREAD = 4, TILE = SCAN_THREADS * PER_THREAD;
constexpr int EXPAND_THREADS = 256, POSITIONS = 4;  // a workgroup writes 4 KiB of A' and 4 KiB of S'
static_assert(mult_section_rows(1) % PER_THREAD == 0 && mult_section_rows(2) % TILE == 0, "a thread's four bins lie in one section");

struct BuildParams {
    const uint32_t *mult;  // [n_sets][MULT_BINS]
    uint32_t *a, *s;       // [n_sets][5][2^k]
    uint32_t *ws;          // [n_sets][PERM_WS_WORDS]
    uint64_t *report;      // aesw_perm_report as 3 x u64
    uint32_t k, n_sets, u, pad_row;
};

// Inclusive scan over the wave.
template <class Op>
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane, Op op) {
#pragma unroll
    for (int d = 1; d < LANES; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, LANES);
        if (lane >= (uint32_t)d) v = op(o, v);
    }
    return v;
}

// What lies in front of this thread's `v` in the workgroup, `carry` included; `carry` then takes the workgroup's total in.  One
// barrier: the caller alternates between two `totals` arrays, so that the barrier of the other one separates a read here from
// the next write.
template <class Op>
__device__ __forceinline__ uint32_t block_scan_before(uint32_t v, uint32_t *totals, uint32_t lane, uint32_t wave, uint32_t &carry, Op op) {
    const uint32_t inc = wave_scan(v, lane, op);
    if (lane == LANES - 1) totals[wave] = inc;
    const uint32_t left = __shfl_up(inc, 1, LANES);
    __syncthreads();
    uint32_t before = carry, total = carry;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)SCAN_WAVES; ++w) {
        const uint32_t t = totals[w];
        if (w < wave) before = op(before, t);
        total = op(total, t);
    }
    carry = total;
    return lane ? op(before, left) : before;
}

// grid: x = the argument, set * 5 + tag - 1
__global__ void __launch_bounds__(SCAN_THREADS) perm_scan_kernel(const BuildParams p) {
    __shared__ uint32_t s_sum[SCAN_WAVES], s_used[SCAN_WAVES];
    const uint32_t set = blockIdx.x / PERM_TAGS, tag = blockIdx.x % PERM_TAGS + 1, u = p.u;
    const uint32_t first = mult_section_first(tag), rows = mult_section_rows(tag);
    const uint32_t *hist = p.mult + (uint64_t)set * MULT_BINS + first;  // 4-byte aligned only: a set has an odd number of bins
    uint32_t *ws = p.ws + (uint64_t)set * PERM_WS_WORDS;
    uint32_t *start = ws + perm_ws_arrays(tag), *used = start + rows, *unused = used + rows;
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const auto sat = [u](uint32_t x, uint32_t y) { return perm_sat_add(x, y, u); };
    const auto add = [](uint32_t x, uint32_t y) { return x + y; };
    const auto load = [&](uint32_t j0, uint32_t *h) {
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) h[q] = j0 < rows ? hist[j0 + q] : 0u;
    };
    uint32_t sum = 0, d = 0;  // the clipped sum and the rows with a count of everything in front of the tile
    uint32_t next[PER_THREAD];
    load(threadIdx.x * PER_THREAD, next);
    for (uint32_t base = 0; base < rows; base += TILE) {
        const uint32_t j0 = base + threadIdx.x * PER_THREAD;
        uint32_t h[PER_THREAD], b[PER_THREAD + 1];
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) h[q] = perm_clip(next[q], u);
        if (base + TILE < rows) load(j0 + TILE, next);  // in flight while this tile is scanned
        b[0] = sat(sat(h[0], h[1]), sat(h[2], h[3]));
        b[0] = block_scan_before(b[0], s_sum, lane, wave, sum, sat);
        uint32_t flags = 0, n_used = 0;
        u32x4 st;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            b[q + 1] = sat(b[q], h[q]);
            st[q] = perm_start(b[q], u);
            if (perm_start(b[q + 1], u) > st[q]) { flags |= 1u << q; ++n_used; }
        }
        uint32_t c = block_scan_before(n_used, s_used, lane, wave, d, add);
        if (j0 < rows) {
            u32x4 us;
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                if (flags >> q & 1u) ++c;
                else unused[j0 + q - c] = first + j0 + q;
                us[q] = c;
            }
            *reinterpret_cast<u32x4 *>(start + j0) = st;
            *reinterpret_cast<u32x4 *>(used + j0) = us;
        }
    }
    if (threadIdx.x == 0) {
        const uint32_t z = perm_start(sum, u);
        const u32x4 sc = {z, d, z < u ? 1u : 0u, sum > u ? 1u : 0u};
        *reinterpret_cast<u32x4 *>(ws + perm_ws_scalars(tag)) = sc;
    }
}

// The report, by one workgroup of EXPAND_THREADS threads, all of them here: how many arguments overflowed and the smallest of them.
__device__ __forceinline__ void write_report(const BuildParams &p) {
    __shared__ unsigned long long s_first[EXPAND_THREADS / LANES];
    __shared__ uint32_t s_count[1][EXPAND_THREADS / LANES];
    const uint32_t n_args = p.n_sets * PERM_TAGS;
    uint32_t count[1] = {0};
    unsigned long long firstv = ~0ull;
    for (uint32_t i = threadIdx.x; i < n_args; i += EXPAND_THREADS) {
        const uint32_t set = i / PERM_TAGS, tag = i % PERM_TAGS + 1;
        if (p.ws[(uint64_t)set * PERM_WS_WORDS + perm_ws_scalars(tag) + 3]) {
            ++count[0];
            const unsigned long long id = (unsigned long long)set * 8 + tag;
            firstv = id < firstv ? id : firstv;
        }
    }
    workgroup_fold(count, firstv, s_count, s_first, threadIdx.x);
    if (threadIdx.x == 0) { p.report[0] = n_args; p.report[1] = count[0]; p.report[2] = firstv; }
}

// grid: x = 1 024 positions of an argument, y = the argument
__global__ void __launch_bounds__(EXPAND_THREADS) perm_expand_kernel(const BuildParams p) {
    if (blockIdx.x == 0 && blockIdx.y == 0) write_report(p);
    const uint32_t set = blockIdx.y / PERM_TAGS, tag = blockIdx.y % PERM_TAGS + 1;
    const uint32_t i0 = (blockIdx.x * EXPAND_THREADS + threadIdx.x) * POSITIONS;
    if (i0 >= p.u) return;
    const PermArgument a = perm_argument(p.ws + (uint64_t)set * PERM_WS_WORDS, tag, p.u, p.pad_row);
    const uint32_t n = p.u - i0 < (uint32_t)POSITIONS ? p.u - i0 : (uint32_t)POSITIONS, z = a.sc.z;
    // the rows of the first and of the last of the lane's positions in front of the all-zero run; the ones between lie between
    uint32_t j = 0, at = 0, j_last = 0;
    if (i0 < z) {
        j = perm_search(a.start, i0, 0, a.rows, at);
        const uint32_t i_last = i0 + n - 1 < z ? i0 + n - 1 : z - 1;
        uint32_t at_last = at;
        j_last = i_last > i0 ? perm_search(a.start, i_last, j, a.rows, at_last) : j;
    }
    u32x4 av, sv;
#pragma unroll
    for (int q = 0; q < POSITIONS; ++q) {
        const uint32_t i = i0 + q;
        av[q] = sv[q] = 0;
        if ((uint32_t)q < n) {
            if (q && i < z && j != j_last) j = perm_search(a.start, i, j, j_last + 1, at);
            av[q] = i < z ? a.first + j : MULT_ZERO_ROW;
            sv[q] = perm_table_cell(a, i, j, at);
        }
    }
    const uint64_t o = ((uint64_t)blockIdx.y << p.k) + i0;
    if (n == (uint32_t)POSITIONS) {
        __builtin_nontemporal_store(av, reinterpret_cast<u32x4 *>(p.a + o));
        __builtin_nontemporal_store(sv, reinterpret_cast<u32x4 *>(p.s + o));
    } else {  // the u % 4 tail: word by word, and nothing behind it
#pragma unroll
        for (int q = 0; q < POSITIONS - 1; ++q)
            if ((uint32_t)q < n) {
                __builtin_nontemporal_store(av[q], p.a + o + q);
                __builtin_nontemporal_store(sv[q], p.s + o + q);
            }
    }
}

// One lane writes one 16-byte half cell; a workgroup writes 4 KiB and exits.
template <int NT>
__global__ void __launch_bounds__(256) perm_gather_fr_kernel(const uint32_t *__restrict__ index, uint64_t n_cells, const u32x4 *__restrict__ table, u32x4 *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells * 2) return;
    const uint32_t r = index[i >> 1];
    u32x4 v = {0, 0, 0, 0};
    if (r < MULT_BINS) v = table[(uint64_t)r * 2 + (uint32_t)(i & 1)];
    gstore<NT>(out + i, v);
}

constexpr uint64_t MAX_GATHER_CELLS = 1ull << 36;

}  // namespace aesw_perm

extern "C" {

size_t aesw_perm_workspace_bytes(uint32_t n_sets) {
    return aesw::mult_sets_ok(n_sets) ? (size_t)n_sets * aesw::PERM_WS_WORDS * sizeof(uint32_t) : 0;
}

int aesw_perm_build_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row, const uint32_t *d_mult, uint32_t *d_a,
                           uint32_t *d_s, void *d_workspace, aesw_perm_report *d_report, void *stream) {
    using namespace aesw_perm;
    static_assert(sizeof(aesw_perm_report) == 3 * sizeof(uint64_t), "the kernel addresses the report as three u64");
    static_assert(AESW_PERM_ARGUMENTS == PERM_TAGS, "one argument per tag");
    const char *const call = "aesw_perm_build_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!perm_k_ok(k)) return refuse(ctx, call, "k must be 17 ... 30 (2^k rows hold the table)");
    if (const char *why = bad_sets(n_sets)) return refuse(ctx, call, why);
    if (!perm_rows_ok(k, n_rows)) return refuse(ctx, call, "n_rows must be 66561 ... 2^k");
    if (pad_row >= MULT_BINS) return refuse(ctx, call, "pad_row must be a table row, 0 ... 66560");
    if (!d_mult || !aligned_to(d_mult, 16)) return refuse(ctx, call, "d_mult must be there and 16-byte aligned");
    if (!d_a || !d_s || !aligned_to(d_a, 16) || !aligned_to(d_s, 16)) return refuse(ctx, call, "d_a and d_s must be there and 16-byte aligned");
    if (!d_workspace || !aligned_to(d_workspace, 16)) return refuse(ctx, call, "d_workspace must be there and 16-byte aligned");
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    BuildParams p{};
    p.mult = d_mult; p.a = d_a; p.s = d_s;
    p.ws = static_cast<uint32_t *>(d_workspace);
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.k = k; p.n_sets = n_sets; p.u = n_rows; p.pad_row = pad_row;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned n_args = n_sets * PERM_TAGS, per_block = EXPAND_THREADS * POSITIONS;
    hipLaunchKernelGGL(perm_scan_kernel, dim3(n_args), dim3(SCAN_THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(perm_expand_kernel, dim3((n_rows + per_block - 1) / per_block, n_args), dim3(EXPAND_THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_perm_gather_fr_device(aesw_ctx *ctx, uint64_t n_cells, const uint32_t *d_index, const uint8_t *d_table_fr, uint8_t *d_out_fr, void *stream) {
    using namespace aesw_perm;
    const char *const call = "aesw_perm_gather_fr_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (n_cells > MAX_GATHER_CELLS) return refuse(ctx, call, "n_cells must be at most 2^36");
    if (n_cells == 0) return AESW_OK;
    if (!d_index || !aligned_to(d_index, 4)) return refuse(ctx, call, "d_index must be there and 4-byte aligned");
    if (!d_table_fr || !d_out_fr || !aligned_to(d_table_fr, 16) || !aligned_to(d_out_fr, 16))
        return refuse(ctx, call, "d_table_fr and d_out_fr must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n_cells * 2 + 255) / 256));
    const u32x4 *table = reinterpret_cast<const u32x4 *>(d_table_fr);
    u32x4 *out = reinterpret_cast<u32x4 *>(d_out_fr);
    with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(perm_gather_fr_kernel<AESW_V(n)>, grid, dim3(256), 0, s, d_index, n_cells, table, out); });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
