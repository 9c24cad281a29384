// sigma/aesw_sigma.hip -- libaesw_sigma.so (include/aesw_sigma.h): the grand products of halo2's permutation argument.
// The field is aesw_fr.h's and the rules -- the constants, the cell index, the power tables, the sets, the chunks, the workspace,
// Assembly::copy -- are aesw_sigma.h's; nothing of either is restated here.  Z needs no inversion per row: with NP the prefix
// product of a set's numerators and SP the suffix product of its denominators (a zero one skipped),
//   Z_s[i] = Z_s[0] * NP[i] * SP[i] * inv(SP[0]),   and zero behind the set's first zero denominator.
// What is here:
//   * sigma_tables_kernel: a thread raises omega or delta to one power;
//   * sigma_prepare_kernel: beta * delta^c for every column, so that a label costs two products;
//   * sigma_chunk_kernel: a workgroup multiplies the numerators and the denominators of its chunk of one set into two cells and
//     counts the zero denominators and the mapping entries out of range;
//   * sigma_carry_kernel: one workgroup per set turns the chunks' numerators into exclusive prefixes and their denominators into
//     exclusive suffixes, in place, and inverts the set's whole denominator -- the one fr_inv of a set;
//   * sigma_chain_kernel: one workgroup chains the sets (halo2's last_z), writes the closing cells, every set's scale and the report;
//   * sigma_scan_kernel<NT>: a workgroup makes the terms of its chunk again, scans the numerators upwards and the denominators
//     downwards -- in the lane, across the wave by shuffles, across waves through LDS -- and stores Z through aesw_store.h's flavour;
//   * the entry points, the host functions and the checks that are theirs alone.
// How a cell lies in memory, moves between lanes and is scanned over a wave is aesw_fr_dev.h's.
// No atomic, no look-back flag, nothing to reset: the passes are ordered by the stream and every output word is stored once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../../include/aesw_sigma.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_sigma.h"

namespace aesw_sigma {
using namespace aesw;

constexpr int THREADS = SIGMA_THREADS, ROWS = SIGMA_ROWS_PER_LANE, WAVES = THREADS / LANES;
static_assert(sizeof(Fr) == 32 && sizeof(aesw_sigma_report) == 6 * sizeof(uint64_t), "a cell is two 16-byte pieces; the kernels address the report as u64 words");
static_assert(sizeof(aesw_copy_edge) == 8, "the edges are read as include/aesw.h lays them out");

// Which launches the product call enqueues: all of them, except in a measurement variant built with -DAESW_SIGMA_PASSES=<mask>
// (tests/test_perf_sigma.py prices one kernel at a time that way; such a library's outputs are of no use).
#ifndef AESW_SIGMA_PASSES
#define AESW_SIGMA_PASSES 0x1f
#endif
constexpr unsigned PASSES = AESW_SIGMA_PASSES, PASS_PREPARE = 1, PASS_CHUNK = 2, PASS_CARRY = 4, PASS_CHAIN = 8, PASS_SCAN = 16;

// ---- the power tables ---------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(THREADS) sigma_tables_kernel(u32x4 *__restrict__ out, uint32_t k, uint32_t cells) {
    const uint32_t at = blockIdx.x * THREADS + threadIdx.x;
    if (at < cells) store_cell<0>(cell_at(out, at), sigma_table_cell(k, at));
}

// ---- the product ----------------------------------------------------------------------------------------------------------------

struct ProductParams {
    const uint8_t *advice, *fixed;  // [n_advice][2^k], [n_fixed][2^k]
    const uint32_t *source, *map;   // [n_cols], [n_cols][2^k]
    const u32x4 *low, *high, *delta, *fr_lut;
    const u32x4 *beta, *gamma;
    u32x4 *z, *closing;
    u32x4 *bd, *num, *den, *set_cells, *chunk_words, *set_words;  // the workspace (aesw_sigma.h)
    uint64_t *report;
    uint32_t k, n_cols, chunk_len, n_rows, n_advice, n_fixed, last_row, stride, sets;
};

__global__ void __launch_bounds__(THREADS) sigma_prepare_kernel(const ProductParams p) {
    const uint32_t c = blockIdx.x * THREADS + threadIdx.x;
    if (c < p.n_cols) store_cell<0>(cell_at(p.bd, c), fr_mul(load_cell(p.beta), load_cell(cell_at(p.delta, c))));
}

// The numerators and the denominators of the lane's rows i0 ... i0 + ROWS - 1 of set `set` -- 1 at and behind n_rows, and 1 for a
// zero denominator, which is counted instead.  i0 < 2^k, a multiple of ROWS.  Five products per column and row, one per row.
__device__ __forceinline__ void lane_terms(const ProductParams &p, uint32_t set, uint32_t i0, Fr (&num)[ROWS], Fr (&den)[ROWS], uint32_t &zeros, uint32_t &first,
                                           uint32_t &out_of_range) {
#pragma unroll
    for (int q = 0; q < ROWS; ++q) num[q] = den[q] = FR_ONE;
    zeros = 0;
    first = ~0u;
    out_of_range = 0;
    if (i0 >= p.n_rows) return;
    const Fr gamma = load_cell(p.gamma);
    Fr w[ROWS];  // omega^(i0 + q): the rows of a lane share the high cell
    {
        const Fr high = load_cell(cell_at(p.high, sigma_high_index(i0)));
        fr_unrolled<ROWS>([&](auto at) {
            constexpr int q = decltype(at)::value;
            w[q] = fr_mul(load_cell(cell_at(p.low, sigma_low_index(i0) + q)), high);
        });
    }
    const uint32_t end = sigma_set_end(set, p.chunk_len, p.n_cols);
#pragma unroll 1
    for (uint32_t c = sigma_set_first(set, p.chunk_len); c < end; ++c) {
        const Fr bd = load_cell(cell_at(p.bd, c));
        const uint32_t src = p.source[c];  // one per workgroup
        const uint8_t *col = src < p.n_advice ? p.advice + ((uint64_t)src << p.k) : src - p.n_advice < p.n_fixed ? p.fixed + ((uint64_t)(src - p.n_advice) << p.k) : nullptr;
        const uint32_t bytes = col ? *reinterpret_cast<const uint32_t *>(col + i0) : 0u;
        const u32x4 cells = *reinterpret_cast<const u32x4 *>(p.map + ((uint64_t)c << p.k) + i0);
        fr_unrolled<ROWS>([&](auto at) {
            constexpr int q = decltype(at)::value;
            if (i0 + q < p.n_rows) {
                const Fr vg = fr_add(load_cell(cell_at(p.fr_lut, bytes >> (8 * q) & 255u)), gamma);
                const Fr n = fr_add(vg, fr_mul(bd, w[q]));
                num[q] = fr_mul(num[q], n);
                const uint32_t m = cells[q];
                Fr d = n;  // a cell that maps to itself, and an entry out of range, which reads as one
                if (!sigma_cell_in_range(p.k, p.n_cols, m)) {
                    ++out_of_range;
                } else if (m != sigma_cell_index(p.k, c, i0 + q)) {
                    const uint32_t row = sigma_cell_row(p.k, m);
                    const Fr label = fr_mul(load_cell(cell_at(p.low, sigma_low_index(row))), load_cell(cell_at(p.high, sigma_high_index(row))));
                    d = fr_add(vg, fr_mul(load_cell(cell_at(p.bd, sigma_cell_col(p.k, m))), label));
                }
                den[q] = fr_mul(den[q], d);
            }
        });
    }
    fr_unrolled<ROWS>([&](auto at) {
        constexpr int q = ROWS - 1 - decltype(at)::value;  // downwards: `first` ends as the lowest row
        if (fr_is_zero(den[q])) {
            den[q] = FR_ONE;
            ++zeros;
            first = i0 + q;
        }
    });
}

// grid: x = the chunk, y = the set
__global__ void __launch_bounds__(THREADS) sigma_chunk_kernel(const ProductParams p) {
    __shared__ Fr s_num[WAVES], s_den[WAVES];
    __shared__ uint32_t s_sums[2][WAVES];
    __shared__ unsigned long long s_first[WAVES];
    const uint32_t set = blockIdx.y, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    Fr num[ROWS], den[ROWS];
    uint32_t sums[2], first_row;
    lane_terms(p, set, blockIdx.x * SIGMA_CHUNK + threadIdx.x * ROWS, num, den, sums[0], first_row, sums[1]);
    Fr n = num[0], d = den[0];
    fr_unrolled<ROWS - 1>([&](auto at) {
        n = fr_mul(n, num[decltype(at)::value + 1]);
        d = fr_mul(d, den[decltype(at)::value + 1]);
    });
#pragma unroll 1
    for (int o = LANES / 2; o; o >>= 1) {  // the field is commutative: a butterfly will do
        n = fr_mul(n, shfl_xor_cell(n, o));
        d = fr_mul(d, shfl_xor_cell(d, o));
    }
    if (lane == 0) {
        s_num[wave] = n;
        s_den[wave] = d;
    }
    unsigned long long first = first_row == ~0u ? ~0ull : first_row;
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);  // joins the workgroup: the waves' cells are there behind it
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int w = 1; w < WAVES; ++w) {
            n = fr_mul(n, s_num[w]);
            d = fr_mul(d, s_den[w]);
        }
        const uint64_t at = (uint64_t)set * p.stride + blockIdx.x;
        store_cell<0>(cell_at(p.num, at), n);
        store_cell<0>(cell_at(p.den, at), d);
        p.chunk_words[at] = u32x4{sums[0], (uint32_t)first, sums[1], 0u};  // ~0ull ends as ~0u
    }
}

// One cell per chunk of a set -> its exclusive scan, in place, 256 chunks a turn: upwards (the product of the chunks below) or,
// REVERSED, downwards (that of the chunks above).  Returns the product of all of them, in every thread.
template <bool REVERSED>
__device__ __forceinline__ Fr scan_chunks(u32x4 *cells, uint32_t chunks, Fr (&s_wave)[WAVES], uint32_t lane, uint32_t wave) {
    Fr running = FR_ONE;  // the product of every turn before this one
    for (uint32_t turn = 0; turn < chunks; turn += THREADS) {
        const uint32_t j = turn + threadIdx.x;  // the place in scan order
        const uint32_t i = j < chunks ? (REVERSED ? chunks - 1u - j : j) : 0u;
        const Fr incl = wave_scan_up(j < chunks ? load_cell(cell_at(cells, i)) : FR_ONE, lane);
        Fr excl = shfl_up_cell(incl, 1);
        if (lane == 0) excl = FR_ONE;
        if (lane == LANES - 1) s_wave[wave] = incl;
        __syncthreads();
        Fr base = running;
#pragma unroll 1
        for (uint32_t w = 0; w < WAVES; ++w) {
            if (w == wave) base = running;  // what lies before this wave
            running = fr_mul(running, s_wave[w]);
        }
        if (j < chunks) store_cell<0>(cell_at(cells, i), fr_mul(base, excl));
        __syncthreads();  // s_wave is written again next turn
    }
    return running;
}

// grid: x = the set
__global__ void __launch_bounds__(THREADS) sigma_carry_kernel(const ProductParams p, uint32_t chunks) {
    __shared__ Fr s_wave[WAVES];
    __shared__ uint32_t s_sums[2][WAVES];
    __shared__ unsigned long long s_first[WAVES];
    const uint32_t set = blockIdx.x, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const uint64_t at = (uint64_t)set * p.stride;
    const Fr n = scan_chunks<false>(cell_at(p.num, at), chunks, s_wave, lane, wave);
    const Fr d = scan_chunks<true>(cell_at(p.den, at), chunks, s_wave, lane, wave);
    uint32_t sums[2] = {0, 0};  // a set has at most 2^28 rows of at most 8 columns: both fit
    unsigned long long first = ~0ull;
    for (uint32_t i = threadIdx.x; i < chunks; i += THREADS) {
        const u32x4 v = p.chunk_words[at + i];
        sums[0] += v[0];
        sums[1] += v[2];
        const unsigned long long f = v[1] == ~0u ? ~0ull : v[1];
        first = f < first ? f : first;
    }
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) {
        const Fr inv = fr_inv(d);  // the one inversion of the set: d is a product of non-zero denominators
        store_cell<0>(cell_at(p.set_cells, set * 2ull), fr_mul(n, inv));
        store_cell<0>(cell_at(p.set_cells, set * 2ull + 1), inv);
        p.set_words[set] = u32x4{sums[0], (uint32_t)first, sums[1], 0u};
    }
}

// one workgroup: Z_s[0] of every set (halo2's last_z), the closing cells, the scale and the rows a set keeps, the report
__global__ void __launch_bounds__(THREADS) sigma_chain_kernel(const ProductParams p) {
    __shared__ Fr s_wave[WAVES];
    __shared__ unsigned long long s_sums[2][WAVES], s_first[WAVES];
    const uint32_t lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const bool ok = fr_is_canonical(load_cell(p.beta)) && fr_is_canonical(load_cell(p.gamma));
    unsigned long long sums[2] = {0, 0}, first = ~0ull;  // zero terms, entries out of range
    Fr running = FR_ONE;                                 // Z at the first row of this turn's first set
    for (uint32_t turn = 0; turn < p.sets; turn += THREADS) {
        const uint32_t s = turn + threadIdx.x;
        const bool active = s < p.sets;
        const u32x4 words = active ? p.set_words[s] : u32x4{0u, ~0u, 0u, 0u};
        // what the set multiplies Z by over all its rows: num / den, and 0 behind a zero term
        const Fr ratio = !active ? FR_ONE : words[0] ? FR_ZERO : load_cell(cell_at(p.set_cells, s * 2ull));
        const Fr incl = wave_scan_up(ratio, lane);
        Fr excl = shfl_up_cell(incl, 1);
        if (lane == 0) excl = FR_ONE;
        if (lane == LANES - 1) s_wave[wave] = incl;
        __syncthreads();
        Fr base = running;
#pragma unroll 1
        for (uint32_t w = 0; w < WAVES; ++w) {
            if (w == wave) base = running;
            running = fr_mul(running, s_wave[w]);
        }
        if (active) {
            Fr z0 = fr_mul(base, excl);
            Fr closing = fr_mul(z0, ratio);
            if (!ok) z0 = closing = FR_ZERO;
            store_cell<0>(cell_at(p.closing, s), closing);
            const Fr inv = load_cell(cell_at(p.set_cells, s * 2ull + 1));
            store_cell<0>(cell_at(p.set_cells, s * 2ull), fr_mul(z0, inv));  // the scale: this thread alone has read the ratio
            p.set_words[s] = u32x4{words[0], words[1], words[2], !ok ? 0u : words[0] ? words[1] + 1u : ~0u};
            sums[0] += words[0];
            sums[1] += words[2];
            const unsigned long long f = words[0] ? ((unsigned long long)s << p.k) + words[1] : ~0ull;
            first = f < first ? f : first;
        }
        __syncthreads();
    }
    for (uint32_t c = threadIdx.x; c < p.n_cols; c += THREADS) sums[1] += (uint64_t)p.source[c] >= (uint64_t)p.n_advice + p.n_fixed ? 1u : 0u;
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) {
        p.report[0] = p.sets;
        p.report[1] = ok && fr_eq(running, FR_ONE) ? 0u : 1u;
        p.report[2] = ok ? sums[0] : 0u;
        p.report[3] = ok ? first : ~0ull;
        p.report[4] = sums[1];
        p.report[5] = ok ? 0u : 1u;
    }
}

// grid: x = the chunk, y = the set.  A lane writes 32 * ROWS contiguous bytes.
template <int NT>
__global__ void __launch_bounds__(THREADS) sigma_scan_kernel(const ProductParams p) {
    __shared__ Fr s_num[WAVES], s_den[WAVES];
    const uint32_t set = blockIdx.y, lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
    const uint32_t i0 = blockIdx.x * SIGMA_CHUNK + threadIdx.x * ROWS;
    Fr num[ROWS], den[ROWS];
    uint32_t zeros, first_row, out_of_range;  // the chunk kernel's to report
    lane_terms(p, set, i0, num, den, zeros, first_row, out_of_range);
    fr_unrolled<ROWS - 1>([&](auto at) {
        constexpr int q = decltype(at)::value;
        num[q + 1] = fr_mul(num[q], num[q + 1]);                        // inclusive upwards, in the lane
        den[ROWS - 2 - q] = fr_mul(den[ROWS - 2 - q], den[ROWS - 1 - q]);  // inclusive downwards
    });
    const Fr incl_n = wave_scan_up(num[ROWS - 1], lane), incl_d = wave_scan_down(den[0], lane);
    Fr excl_n = shfl_up_cell(incl_n, 1), excl_d = shfl_down_cell(incl_d, 1);
    if (lane == 0) excl_n = FR_ONE;
    if (lane == LANES - 1) excl_d = FR_ONE;
    if (lane == LANES - 1) s_num[wave] = incl_n;
    if (lane == 0) s_den[wave] = incl_d;
    __syncthreads();
    const uint64_t at = (uint64_t)set * p.stride + blockIdx.x;
    Fr below = fr_mul(load_cell(cell_at(p.set_cells, set * 2ull)), load_cell(cell_at(p.num, at)));  // Z_s[0] / SP[0] * NP at the chunk's first row
#pragma unroll 1
    for (uint32_t w = 0; w < wave; ++w) below = fr_mul(below, s_num[w]);
    Fr above = load_cell(cell_at(p.den, at));  // SP behind the chunk's last row
#pragma unroll 1
    for (uint32_t w = wave + 1; w < (uint32_t)WAVES; ++w) above = fr_mul(above, s_den[w]);
    const Fr base = fr_mul(fr_mul(below, excl_n), fr_mul(above, excl_d));
    const uint32_t keep = p.set_words[set][3];  // rows below it keep their value, the others are zero
    u32x4 *z = cell_at(p.z, ((uint64_t)set << p.k) + i0);
    fr_unrolled<ROWS>([&](auto at_q) {
        constexpr int q = decltype(at_q)::value;
        if (i0 + q <= p.last_row) {
            Fr v = FR_ZERO;
            if (i0 + q < keep) {
                if constexpr (q == 0) v = fr_mul(base, den[0]);
                else v = fr_mul(base, fr_mul(num[q - 1], den[q]));
            }
            store_cell<NT>(cell_at(z, q), v);
        }
    });
}

}  // namespace aesw_sigma

extern "C" {

uint32_t aesw_sigma_columns(uint32_t n_sets) { return aesw::sigma_columns(n_sets); }

int aesw_sigma_sources_host(uint32_t n_sets, uint32_t *source) {
    if (!source || n_sets < 1 || n_sets > 1024) return AESW_ERR_INVALID_ARG;
    for (uint32_t c = 0; c < aesw::sigma_columns(n_sets); ++c) source[c] = aesw::sigma_source_of_column(n_sets, c);
    return AESW_OK;
}

int aesw_sigma_mapping_host(uint32_t k, uint32_t n_sets, uint32_t n_blocks, uint32_t *map) {
    using namespace aesw;
    if (!map || n_sets < 1 || n_sets > 1024 || !sigma_shape_ok(k, sigma_columns(n_sets))) return AESW_ERR_INVALID_ARG;
    if (n_blocks > aesw_block_capacity(k, n_sets)) return AESW_ERR_CAPACITY;
    const uint64_t cells = sigma_cells(k, sigma_columns(n_sets));
    uint32_t *aux = new (std::nothrow) uint32_t[cells], *sizes = new (std::nothrow) uint32_t[cells];
    aesw_copy_edge *key_edges = new (std::nothrow) aesw_copy_edge[AESW_KEY_COPIES], *block_edges = new (std::nothrow) aesw_copy_edge[AESW_BLOCK_COPIES];
    int rc = aux && sizes && key_edges && block_edges ? AESW_OK : AESW_ERR_NOMEM;
    if (rc == AESW_OK) rc = aesw_key_copy_graph(key_edges);
    if (rc == AESW_OK) rc = aesw_block_copy_graph(block_edges);
    if (rc == AESW_OK)
        sigma_build_mapping(k, n_sets, n_blocks, key_edges, AESW_KEY_COPIES, block_edges, AESW_BLOCK_COPIES,
                            [&](uint32_t b, uint32_t *set, uint32_t *row) {
                                uint64_t r = 0;
                                (void)aesw_block_placement(k, n_sets, b, set, &r);  // b is below the capacity: it has a place
                                *row = (uint32_t)r;
                            },
                            map, aux, sizes);
    delete[] aux;
    delete[] sizes;
    delete[] key_edges;
    delete[] block_edges;
    return rc;
}

size_t aesw_sigma_tables_bytes(uint32_t k, uint32_t n_cols) { return (size_t)aesw::sigma_tables_bytes(k, n_cols); }
size_t aesw_sigma_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t chunk_len) { return (size_t)aesw::sigma_workspace_bytes(k, n_cols, chunk_len); }

int aesw_sigma_tables_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint8_t *d_tables, void *stream) {
    using namespace aesw_sigma;
    const char *const call = "aesw_sigma_tables_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!sigma_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28 (the field's 2-adicity is 28)");
    if (!sigma_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 3074");
    if (!sigma_shape_ok(k, n_cols)) return refuse(ctx, call, "n_cols * 2^k must not exceed 2^32 (a cell index is 32 bits)");
    if (!d_tables || !aligned_to(d_tables, 16)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    const uint32_t cells = (uint32_t)sigma_tables_cells(k, n_cols);  // at most 2^15 + 3074
    hipLaunchKernelGGL(sigma_tables_kernel, dim3((cells + THREADS - 1) / THREADS), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<u32x4 *>(d_tables), k, cells);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_sigma_product_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, uint32_t chunk_len, uint32_t n_rows, const uint8_t *d_advice, uint32_t n_advice,
                              const uint8_t *d_fixed, uint32_t n_fixed, const uint32_t *d_source, const uint32_t *d_map, const uint8_t *d_tables,
                              const uint8_t *d_beta, const uint8_t *d_gamma, uint8_t *d_z_fr, uint8_t *d_closing_fr, void *d_workspace, aesw_sigma_report *d_report,
                              void *stream) {
    using namespace aesw_sigma;
    const char *const call = "aesw_sigma_product_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!sigma_k_ok(k)) return refuse(ctx, call, "k must be 10 ... 28 (the field's 2-adicity is 28)");
    if (!sigma_cols_ok(n_cols)) return refuse(ctx, call, "n_cols must be 1 ... 3074");
    if (!sigma_shape_ok(k, n_cols)) return refuse(ctx, call, "n_cols * 2^k must not exceed 2^32 (a cell index is 32 bits)");
    if (!sigma_chunk_len_ok(chunk_len)) return refuse(ctx, call, "chunk_len must be 1 ... 8");
    if (n_rows < 1 || n_rows > (1u << k)) return refuse(ctx, call, "n_rows must be 1 ... 2^k");
    if ((n_advice && !d_advice) || !aligned_to(d_advice, 16)) return refuse(ctx, call, "d_advice must be there (for n_advice > 0) and 16-byte aligned");
    if ((n_fixed && !d_fixed) || !aligned_to(d_fixed, 16)) return refuse(ctx, call, "d_fixed must be there (for n_fixed > 0) and 16-byte aligned");
    if (!d_source || !aligned_to(d_source, 4)) return refuse(ctx, call, "d_source must be there and 4-byte aligned");
    if (!d_map || !aligned_to(d_map, 16)) return refuse(ctx, call, "d_map must be there and 16-byte aligned");
    if (!d_tables || !aligned_to(d_tables, 16)) return refuse(ctx, call, "d_tables must be there and 16-byte aligned");
    if (const char *why = bad_challenges(d_beta, d_gamma)) return refuse(ctx, call, why);
    if (const char *why = bad_product_outputs(d_z_fr, d_closing_fr)) return refuse(ctx, call, why);
    if (const char *why = bad_workspace(d_workspace)) return refuse(ctx, call, why);
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const SigmaWorkspace ws = sigma_workspace(k, n_cols, chunk_len);
    uint8_t *const base = static_cast<uint8_t *>(d_workspace);
    const u32x4 *tables = reinterpret_cast<const u32x4 *>(d_tables);
    ProductParams p{};
    p.advice = d_advice; p.fixed = d_fixed; p.source = d_source; p.map = d_map;
    p.low = tables;
    p.high = tables + (uint64_t)sigma_low_cells(k) * 2;
    p.delta = p.high + (uint64_t)sigma_high_cells(k) * 2;
    p.fr_lut = reinterpret_cast<const u32x4 *>(ctx->d_fr_lut);
    p.beta = reinterpret_cast<const u32x4 *>(d_beta);
    p.gamma = reinterpret_cast<const u32x4 *>(d_gamma);
    p.z = reinterpret_cast<u32x4 *>(d_z_fr);
    p.closing = reinterpret_cast<u32x4 *>(d_closing_fr);
    p.bd = reinterpret_cast<u32x4 *>(base + ws.bd);
    p.num = reinterpret_cast<u32x4 *>(base + ws.num);
    p.den = reinterpret_cast<u32x4 *>(base + ws.den);
    p.set_cells = reinterpret_cast<u32x4 *>(base + ws.set_cells);
    p.chunk_words = reinterpret_cast<u32x4 *>(base + ws.chunk_words);
    p.set_words = reinterpret_cast<u32x4 *>(base + ws.set_words);
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.k = k; p.n_cols = n_cols; p.chunk_len = chunk_len; p.n_rows = n_rows; p.n_advice = n_advice; p.n_fixed = n_fixed;
    p.last_row = sigma_last_row(k, n_rows);
    p.stride = sigma_chunk_stride(k);
    p.sets = sigma_sets(n_cols, chunk_len);
    const uint32_t chunks = sigma_chunks(k, n_rows);  // <= 2^18, and sets <= 3074: both fit a grid
    const dim3 grid(chunks, p.sets);
    if constexpr (PASSES & PASS_PREPARE) hipLaunchKernelGGL(sigma_prepare_kernel, dim3((n_cols + THREADS - 1) / THREADS), dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CHUNK) hipLaunchKernelGGL(sigma_chunk_kernel, grid, dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CARRY) hipLaunchKernelGGL(sigma_carry_kernel, dim3(p.sets), dim3(THREADS), 0, s, p, chunks);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_CHAIN) hipLaunchKernelGGL(sigma_chain_kernel, dim3(1), dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    if constexpr (PASSES & PASS_SCAN) with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(sigma_scan_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, p); });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
