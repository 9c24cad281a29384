// aesw_sigma.h -- the rules of libaesw_sigma.so, once: the field constants of halo2's permutation argument
// (omega_k, delta, derived from the generator 7 at compile time -- none is quoted), how a cell index names a cell, how omega's
// exponent is split over two power tables, which columns a set multiplies, how a set's rows are cut into chunks, the workspace,
// and the order of the permutation's columns in a FixedAes128Config circuit.  One source for the kernels of
// sigma/aesw_sigma.hip, the host mapping code and the CPU tests.  The field is aesw_fr.h's; nothing of it is restated.
// No HIP call and no ROCm include: tests/test_sigma_model.py compiles this header alone with g++.
#pragma once
#include <stdint.h>

#include "aesw_fr.h"

#if defined(__HIPCC__)
#define AESW_SIGMA_HD __host__ __device__ __forceinline__
#else
#define AESW_SIGMA_HD inline
#endif

namespace aesw {

// ---- the field constants ---------------------------------------------------------------------------------------------------
constexpr uint32_t SIGMA_TWO_ADICITY = 28;  // r - 1 = 2^28 * t, t odd
static_assert((FR_MODULUS.l[0] - 1u) % (1u << SIGMA_TWO_ADICITY) == 0 && ((FR_MODULUS.l[0] - 1u) >> SIGMA_TWO_ADICITY) % 2u == 1u,
              "2^28 divides r - 1 and 2^29 does not");

// limb i of t = (r - 1) >> 28
constexpr uint32_t sigma_t_limb(int i) {
    const uint32_t lo = (i == 0 ? FR_MODULUS.l[0] - 1u : FR_MODULUS.l[i]) >> SIGMA_TWO_ADICITY;
    const uint32_t hi = i + 1 < FR_LIMBS ? FR_MODULUS.l[i + 1] << (32 - SIGMA_TWO_ADICITY) : 0u;
    return lo | hi;
}
// a^e for an exponent of eight limbs given by a function of the limb's number: square and multiply, highest bit first
template <class Limb>
constexpr Fr sigma_pow_limbs(const Fr &a, Limb limb) {
    Fr acc = FR_ONE;
    for (int i = FR_LIMBS - 1; i >= 0; --i) {
        const uint32_t e = limb(i);
        for (int b = 31; b >= 0; --b) {
            acc = fr_mul(acc, acc);
            if (e >> b & 1u) acc = fr_mul(acc, a);
        }
    }
    return acc;
}
constexpr Fr sigma_squared(Fr a, uint32_t times) {
    for (uint32_t i = 0; i < times; ++i) a = fr_mul(a, a);
    return a;
}
constexpr Fr sigma_small(uint32_t v) {  // the Montgomery form of a small integer
    Fr acc = FR_ZERO;
    for (uint32_t i = 0; i < v; ++i) acc = fr_add(acc, FR_ONE);
    return acc;
}
constexpr Fr SIGMA_GENERATOR = sigma_small(7);                                      // halo2curves' MULTIPLICATIVE_GENERATOR
constexpr Fr SIGMA_ROOT = sigma_pow_limbs(SIGMA_GENERATOR, sigma_t_limb);           // g^t: of order 2^28
constexpr Fr SIGMA_DELTA = sigma_squared(SIGMA_GENERATOR, SIGMA_TWO_ADICITY);       // g^(2^28): of order t
static_assert(fr_eq(sigma_squared(SIGMA_ROOT, SIGMA_TWO_ADICITY), FR_ONE) && !fr_eq(sigma_squared(SIGMA_ROOT, SIGMA_TWO_ADICITY - 1), FR_ONE),
              "the root of unity has order 2^28 exactly");
static_assert(fr_eq(sigma_pow_limbs(SIGMA_DELTA, sigma_t_limb), FR_ONE) && !fr_eq(SIGMA_DELTA, FR_ONE), "delta^t = 1 and delta is not 1");

// a^e, e a 32-bit exponent: a loop that stays a loop
AESW_SIGMA_HD constexpr Fr fr_pow_u32(const Fr &a, uint32_t e) {
    Fr acc = FR_ONE;
    for (int b = 31; b >= 0; --b) {
        acc = fr_mul(acc, acc);
        if (e >> b & 1u) acc = fr_mul(acc, a);
    }
    return acc;
}
// omega_k = g^((r - 1) / 2^k), k <= 28
AESW_SIGMA_HD constexpr Fr sigma_omega(uint32_t k) {
    Fr w = SIGMA_ROOT;
    for (uint32_t i = k; i < SIGMA_TWO_ADICITY; ++i) w = fr_mul(w, w);
    return w;
}

// ---- bounds -----------------------------------------------------------------------------------------------------------------
constexpr uint32_t SIGMA_MIN_K = 10, SIGMA_MAX_K = SIGMA_TWO_ADICITY, SIGMA_MAX_COLS = 3u * 1024u + 2u, SIGMA_MAX_CHUNK_LEN = 8;
AESW_SIGMA_HD constexpr bool sigma_k_ok(uint32_t k) { return k >= SIGMA_MIN_K && k <= SIGMA_MAX_K; }
AESW_SIGMA_HD constexpr bool sigma_cols_ok(uint32_t n_cols) { return n_cols >= 1 && n_cols <= SIGMA_MAX_COLS; }
AESW_SIGMA_HD constexpr bool sigma_chunk_len_ok(uint32_t chunk_len) { return chunk_len >= 1 && chunk_len <= SIGMA_MAX_CHUNK_LEN; }
// the cells of the permutation: a cell index is one uint32_t, so there are at most 2^32 of them
AESW_SIGMA_HD constexpr uint64_t sigma_cells(uint32_t k, uint32_t n_cols) { return (uint64_t)n_cols << k; }
AESW_SIGMA_HD constexpr bool sigma_shape_ok(uint32_t k, uint32_t n_cols) { return sigma_k_ok(k) && sigma_cols_ok(n_cols) && sigma_cells(k, n_cols) <= (1ull << 32); }

// ---- a cell index ------------------------------------------------------------------------------------------------------------
// map[c][i] = c' * 2^k + i'
AESW_SIGMA_HD constexpr uint32_t sigma_cell_index(uint32_t k, uint32_t col, uint32_t row) { return (col << k) + row; }
AESW_SIGMA_HD constexpr uint32_t sigma_cell_col(uint32_t k, uint32_t m) { return m >> k; }
AESW_SIGMA_HD constexpr uint32_t sigma_cell_row(uint32_t k, uint32_t m) { return m & ((1u << k) - 1u); }
AESW_SIGMA_HD constexpr bool sigma_cell_in_range(uint32_t k, uint32_t n_cols, uint32_t m) { return (uint64_t)m < sigma_cells(k, n_cols); }

// ---- the power tables ---------------------------------------------------------------------------------------------------------
// omega^i = low[i & (2^14 - 1)] * high[i >> 14]: low[j] = omega^j, high[j] = omega^(j * 2^14); then delta^c for c < n_cols.
constexpr uint32_t SIGMA_SPLIT = 14;
AESW_SIGMA_HD constexpr uint32_t sigma_low_cells(uint32_t k) { return 1u << (k < SIGMA_SPLIT ? k : SIGMA_SPLIT); }
AESW_SIGMA_HD constexpr uint32_t sigma_high_cells(uint32_t k) { return k > SIGMA_SPLIT ? 1u << (k - SIGMA_SPLIT) : 1u; }
AESW_SIGMA_HD constexpr uint32_t sigma_low_index(uint32_t row) { return row & ((1u << SIGMA_SPLIT) - 1u); }
AESW_SIGMA_HD constexpr uint32_t sigma_high_index(uint32_t row) { return row >> SIGMA_SPLIT; }
AESW_SIGMA_HD constexpr uint64_t sigma_tables_cells(uint32_t k, uint32_t n_cols) { return (uint64_t)sigma_low_cells(k) + sigma_high_cells(k) + n_cols; }
AESW_SIGMA_HD constexpr uint64_t sigma_tables_bytes(uint32_t k, uint32_t n_cols) { return sigma_shape_ok(k, n_cols) ? sigma_tables_cells(k, n_cols) * sizeof(Fr) : 0u; }
// cell `at` of the tables, as the tables kernel computes it
AESW_SIGMA_HD constexpr Fr sigma_table_cell(uint32_t k, uint32_t at) {
    const uint32_t low = sigma_low_cells(k), high = sigma_high_cells(k);
    if (at < low) return fr_pow_u32(sigma_omega(k), at);
    if (at < low + high) return fr_pow_u32(sigma_omega(k), (at - low) << SIGMA_SPLIT);  // < 2^k: no exponent wraps
    return fr_pow_u32(SIGMA_DELTA, at - low - high);
}
static_assert(sigma_low_cells(28) * sizeof(Fr) <= (1u << 20) && sigma_high_cells(28) * sizeof(Fr) <= (1u << 20), "each power table stays within 1 MiB");

// ---- sets, rows and chunks ------------------------------------------------------------------------------------------------------
AESW_SIGMA_HD constexpr uint32_t sigma_sets(uint32_t n_cols, uint32_t chunk_len) { return (n_cols + chunk_len - 1) / chunk_len; }
AESW_SIGMA_HD constexpr uint32_t sigma_set_first(uint32_t set, uint32_t chunk_len) { return set * chunk_len; }
AESW_SIGMA_HD constexpr uint32_t sigma_set_end(uint32_t set, uint32_t chunk_len, uint32_t n_cols) {
    return (set + 1) * chunk_len < n_cols ? (set + 1) * chunk_len : n_cols;
}

#ifndef AESW_SIGMA_ROWS_PER_LANE
#define AESW_SIGMA_ROWS_PER_LANE 4  // consecutive rows of a set a lane of the chunk and scan kernels owns
#endif
constexpr uint32_t SIGMA_ROWS_PER_LANE = AESW_SIGMA_ROWS_PER_LANE, SIGMA_THREADS = 256, SIGMA_CHUNK = SIGMA_THREADS * SIGMA_ROWS_PER_LANE;
static_assert(SIGMA_ROWS_PER_LANE == 4, "a lane reads its rows of a byte column as one word and of the mapping as one 16-byte load");
static_assert((1u << SIGMA_MIN_K) % SIGMA_CHUNK == 0, "the smallest column is whole chunks");
// rows 0 ... last are written: row n_rows holds the closing product where 2^k has a row for it
AESW_SIGMA_HD constexpr uint32_t sigma_last_row(uint32_t k, uint32_t n_rows) { return n_rows < (1u << k) ? n_rows : (1u << k) - 1u; }
AESW_SIGMA_HD constexpr uint32_t sigma_chunks(uint32_t k, uint32_t n_rows) { return sigma_last_row(k, n_rows) / SIGMA_CHUNK + 1u; }
AESW_SIGMA_HD constexpr uint32_t sigma_chunk_stride(uint32_t k) { return (1u << k) / SIGMA_CHUNK; }
static_assert(sigma_chunks(10, 1024) == 1 && sigma_chunks(11, 1024) == 2 && sigma_chunks(28, 1u << 28) == sigma_chunk_stride(28), "no n_rows needs more chunks than the stride");

// The workspace, in 32-byte cells and then 16-byte words:
//   beta * delta^c            n_cols cells
//   the chunks' numerators    sets * stride cells (their products, then their exclusive prefixes)
//   the chunks' denominators  sets * stride cells (their products, then their exclusive suffixes)
//   the sets' cells           sets * 2 cells (num / den of the whole set and inv(den); then the set's scale)
//   the chunks' counts        sets * stride words {zero terms, first zero row, out-of-range entries, 0}
//   the sets' counts          sets words {zero terms, first zero row, out-of-range entries, rows that keep their value}
struct SigmaWorkspace {
    uint64_t bd, num, den, set_cells, chunk_words, set_words, bytes;  // byte offsets; all multiples of 16
};
AESW_SIGMA_HD constexpr SigmaWorkspace sigma_workspace(uint32_t k, uint32_t n_cols, uint32_t chunk_len) {
    const uint64_t sets = sigma_sets(n_cols, chunk_len), per_set = sigma_chunk_stride(k), cell = sizeof(Fr);
    SigmaWorkspace w{};
    w.bd = 0;
    w.num = w.bd + n_cols * cell;
    w.den = w.num + sets * per_set * cell;
    w.set_cells = w.den + sets * per_set * cell;
    w.chunk_words = w.set_cells + sets * 2 * cell;
    w.set_words = w.chunk_words + sets * per_set * 16u;
    w.bytes = w.set_words + sets * 16u;
    return w;
}
AESW_SIGMA_HD constexpr uint64_t sigma_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t chunk_len) {
    return sigma_shape_ok(k, n_cols) && sigma_chunk_len_ok(chunk_len) ? sigma_workspace(k, n_cols, chunk_len).bytes : 0u;
}

// ---- the permutation's columns in a FixedAes128Config<k, n_sets> circuit ---------------------------------------------------------
// configure() enables equality in the order  x0 y0 z0 words rcon x1 y1 z1 ...  (the key schedule's configure runs first: set 0's
// three columns, words_column, then enable_constant on the fixed round_constants column; the other sets follow).  The assembled
// advice columns lie in another order: set i at 3 i ... 3 i + 2, words_column last at 3 n_sets; the fixed column is numbered
// 3 n_sets + 1 here, the first one behind the advice columns.
AESW_SIGMA_HD constexpr uint32_t sigma_columns(uint32_t n_sets) { return 3u * n_sets + 2u; }
AESW_SIGMA_HD constexpr uint32_t sigma_source_of_column(uint32_t n_sets, uint32_t c) {
    return c < 3u ? c : c == 3u ? 3u * n_sets : c == 4u ? 3u * n_sets + 1u : c - 2u;
}
// the permutation column of an assembled advice column (a <= 3 n_sets)
AESW_SIGMA_HD constexpr uint32_t sigma_column_of_advice(uint32_t n_sets, uint32_t a) { return a < 3u ? a : a == 3u * n_sets ? 3u : a + 2u; }

// ---- sigma from the copies (keygen, host) ------------------------------------------------------------------------------------------
// halo2's permutation::keygen::Assembly::copy restated over cell indices.  mapping starts as the identity, aux[cell] = cell (every
// cell the head of its own cycle), sizes[cell] = 1.
inline void sigma_assembly_copy(uint32_t *mapping, uint32_t *aux, uint32_t *sizes, uint32_t left, uint32_t right) {
    if (aux[left] == aux[right]) return;
    if (sizes[aux[left]] < sizes[aux[right]]) {  // the larger cycle is "left"; on equal sizes the call's left stays left
        const uint32_t t = left;
        left = right;
        right = t;
    }
    const uint32_t head = aux[left];
    sizes[head] += sizes[aux[right]];
    uint32_t i = right;
    do {  // once round the right cycle
        aux[i] = head;
        i = mapping[i];
    } while (i != right);
    const uint32_t t = mapping[left];
    mapping[left] = mapping[right];
    mapping[right] = t;
}

// The cell of a copy edge's end (include/aesw.h, aesw_copy_edge): space 0 the block's slab in column set `set` from row
// `block_row`, 1 the key slab (set 0, rows 0 ... 399), 2 words_column.
AESW_SIGMA_HD constexpr uint32_t sigma_edge_cell(uint32_t k, uint32_t n_sets, uint32_t space, uint32_t col, uint32_t row, uint32_t set, uint32_t block_row) {
    const uint32_t advice = space == 0 ? 3u * set + col : space == 1 ? col : 3u * n_sets;
    return sigma_cell_index(k, sigma_column_of_advice(n_sets, advice), space == 0 ? block_row + row : row);
}

// The mapping of a circuit with one schedule_key and n_blocks encrypt calls, in synthesize()'s call order.  Edge: aesw_copy_edge.
// place(b, &set, &row): aesw_block_placement.  copy(left, right): left is the new cell (dst), right the copied one (src), as
// AssignedCell::copy_advice calls constrain_equal.  aux and sizes: sigma_cells(k, columns) words each, the caller's.
template <class Edge, class Place>
inline void sigma_build_mapping(uint32_t k, uint32_t n_sets, uint32_t n_blocks, const Edge *key_edges, uint32_t n_key_edges, const Edge *block_edges,
                                uint32_t n_block_edges, Place &&place, uint32_t *mapping, uint32_t *aux, uint32_t *sizes) {
    const uint64_t cells = sigma_cells(k, sigma_columns(n_sets));
    for (uint64_t i = 0; i < cells; ++i) {
        mapping[i] = aux[i] = (uint32_t)i;
        sizes[i] = 1;
    }
    const auto apply = [&](const Edge *edges, uint32_t n, uint32_t set, uint32_t row) {
        for (uint32_t e = 0; e < n; ++e)
            sigma_assembly_copy(mapping, aux, sizes, sigma_edge_cell(k, n_sets, edges[e].dst_space, edges[e].dst_col, edges[e].dst_row, set, row),
                                sigma_edge_cell(k, n_sets, edges[e].src_space, edges[e].src_col, edges[e].src_row, set, row));
    };
    apply(key_edges, n_key_edges, 0, 0);
    for (uint32_t b = 0; b < n_blocks; ++b) {
        uint32_t set = 0, row = 0;
        place(b, &set, &row);
        apply(block_edges, n_block_edges, set, row);
    }
}

}  // namespace aesw
