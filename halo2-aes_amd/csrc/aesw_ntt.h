// aesw_ntt.h -- the rules of libaesw_ntt.so, once: the number-theoretic transform over bn256's Fr that moves a
// column between Lagrange, coefficient and extended-coset form.  Here: the constants (zeta, 1/2, derived from the generator 7 at
// compile time -- none is quoted; omega_k is aesw_sigma.h's), the pass plan of a k, which cell of a column sits in which LDS slot
// of which workgroup, which twiddle a slot takes when it is loaded and which a butterfly takes, the LDS swizzle, the tables and
// the workspace.  One source for the kernels of ntt/aesw_ntt.hip and for the CPU driver of tests/test_ntt_model.py, which runs
// the plan through these very functions.  The field is aesw_fr.h's; nothing of it is restated.
// No HIP call and no ROCm include: the tests compile this header alone with g++.
//
// The transform of size 2^k is radix-2 decimation in time over a bit-reversed load: pass p runs stages s0 + 1 ... s0 + m of it
// (s0 = p * NTT_PASS_LOG, m = min(NTT_PASS_LOG, k - s0)).  A workgroup holds a tile of 2^NTT_PASS_LOG cells in LDS: 2^a
// neighbouring sub-transforms (a = NTT_PASS_LOG - m) of 2^m cells each, the cells of one of them 2^s0 apart in the column.  The
// first pass loads cell bitrev_k(position); a later pass multiplies the cell at slot t of sub-transform `lo` by
// omega_(2^(s0+m))^(lo * bitrev_m(t)) as it loads it (the four-step twiddle), after which its m stages are a plain transform of
// size 2^m whose twiddles are powers of omega_(2^NTT_PASS_LOG): the short table.
#pragma once
#include <stdint.h>

#include "aesw_fr.h"
#include "aesw_sigma.h"

#if defined(__HIPCC__)
#define AESW_NTT_HD __host__ __device__ __forceinline__
#else
#define AESW_NTT_HD inline
#endif

#ifndef AESW_NTT_PASS_LOG
#define AESW_NTT_PASS_LOG 10  // stages a pass runs in LDS; a measurement build overrides it (1: the plain global-memory radix-2)
#endif

namespace aesw {

// ---- bounds -----------------------------------------------------------------------------------------------------------------
constexpr uint32_t NTT_PASS_LOG = AESW_NTT_PASS_LOG, NTT_SLOTS = 1u << NTT_PASS_LOG, NTT_THREADS = 256;
constexpr uint32_t NTT_MIN_K = 10, NTT_MAX_K = SIGMA_TWO_ADICITY, NTT_MAX_COLS = 65535;  // a column is a grid row
static_assert(NTT_PASS_LOG >= 1 && NTT_PASS_LOG <= NTT_MIN_K, "a tile is no larger than the smallest column: 32 KiB of LDS at 10");
AESW_NTT_HD constexpr bool ntt_k_ok(uint32_t k) { return k >= NTT_MIN_K && k <= NTT_MAX_K; }
AESW_NTT_HD constexpr bool ntt_cols_ok(uint32_t n_cols) { return n_cols >= 1 && n_cols <= NTT_MAX_COLS; }
AESW_NTT_HD constexpr bool ntt_shape_ok(uint32_t k, uint32_t n_cols) { return ntt_k_ok(k) && ntt_cols_ok(n_cols); }
AESW_NTT_HD constexpr uint64_t ntt_cells(uint32_t k, uint32_t n_cols) { return (uint64_t)n_cols << k; }  // may pass 2^32

// ---- the constants ------------------------------------------------------------------------------------------------------------
// (r - 1) / 3 by long division, highest limb first
struct NttThird {
    uint32_t limb[FR_LIMBS];
    uint32_t remainder;
};
constexpr NttThird ntt_third() {
    NttThird q{};
    uint64_t rem = 0;
    for (int i = FR_LIMBS - 1; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | (i == 0 ? FR_MODULUS.l[0] - 1u : FR_MODULUS.l[i]);
        q.limb[i] = (uint32_t)(cur / 3u);
        rem = cur % 3u;
    }
    q.remainder = (uint32_t)rem;
    return q;
}
constexpr NttThird NTT_THIRD = ntt_third();
static_assert(NTT_THIRD.remainder == 0, "3 divides r - 1");
constexpr uint32_t ntt_third_limb(int i) { return NTT_THIRD.limb[i]; }
// zeta_sel 0 is g^((r - 1) / 3), zeta_sel 1 its square -- the two primitive cube roots of 1.  Which of them halo2curves calls
// Fr::ZETA is NOT pinned by a test (the crate is not at hand); from memory it is the square, zeta_sel 1.
constexpr Fr NTT_ZETA0 = sigma_pow_limbs(SIGMA_GENERATOR, ntt_third_limb);
constexpr Fr NTT_ZETA1 = fr_mul(NTT_ZETA0, NTT_ZETA0);
static_assert(fr_eq(fr_mul(NTT_ZETA1, NTT_ZETA0), FR_ONE) && !fr_eq(NTT_ZETA0, FR_ONE), "zeta^3 = 1 and zeta is not 1");
static_assert(fr_eq(fr_mul(fr_mul(NTT_ZETA1, NTT_ZETA1), NTT_ZETA1), FR_ONE) && !fr_eq(NTT_ZETA1, FR_ONE) && !fr_eq(NTT_ZETA1, NTT_ZETA0),
              "so is its square, and it is the other one");
constexpr Fr NTT_INV_TWO = fr_inv(fr_add(FR_ONE, FR_ONE));
// zeta0^v, v < 3
AESW_NTT_HD constexpr Fr ntt_zeta0_power(uint32_t v) { return v == 0 ? FR_ONE : v == 1 ? NTT_ZETA0 : NTT_ZETA1; }
// zeta^(index mod 3) as a power v of zeta0, zeta = zeta0^(zeta_sel + 1): what coefficient `index` is multiplied by on the way into
// the coset (halo2's distribute_powers_zeta); `out_of_coset`: its inverse
AESW_NTT_HD constexpr uint32_t ntt_zeta_exponent(uint32_t zeta_sel, uint32_t index, bool out_of_coset) {
    const uint32_t e = (zeta_sel + 1u) * (index % 3u) % 3u;
    return out_of_coset ? (3u - e) % 3u : e;
}

// ---- the pass plan ----------------------------------------------------------------------------------------------------------------
struct NttPass {
    uint32_t s0, m, a;  // stages s0 + 1 ... s0 + m; the tile holds 2^a sub-transforms of 2^m cells
};
AESW_NTT_HD constexpr uint32_t ntt_passes(uint32_t k) { return (k + NTT_PASS_LOG - 1u) / NTT_PASS_LOG; }
AESW_NTT_HD constexpr NttPass ntt_pass(uint32_t k, uint32_t p) {
    const uint32_t s0 = p * NTT_PASS_LOG, m = k - s0 < NTT_PASS_LOG ? k - s0 : NTT_PASS_LOG;
    return NttPass{s0, m, NTT_PASS_LOG - m};
}
// a short pass is never the first one (k >= NTT_PASS_LOG), so the 2^a neighbours exist: a <= s0
static_assert(ntt_passes(10) == (10 + NTT_PASS_LOG - 1) / NTT_PASS_LOG && ntt_pass(28, ntt_passes(28) - 1).s0 + ntt_pass(28, ntt_passes(28) - 1).m == 28, "the stages add up");
AESW_NTT_HD constexpr uint32_t ntt_workgroups(uint32_t k) { return 1u << (k - NTT_PASS_LOG); }  // per column and pass

// the lowest `bits` bits of v reversed (bits 0 ... 28)
AESW_NTT_HD constexpr uint32_t ntt_bitrev(uint32_t v, uint32_t bits) {
    v = (v >> 16) | (v << 16);
    v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
    v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
    v = ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
    return bits ? v >> (32u - bits) : 0u;
}

// LDS slot `slot` of workgroup w: the sub-transform's number within the tile and the cell's place t in it
AESW_NTT_HD constexpr uint32_t ntt_slot_t(const NttPass &q, uint32_t slot) { return slot >> q.a; }
// the sub-transform's place `lo` below 2^s0
AESW_NTT_HD constexpr uint32_t ntt_slot_lo(const NttPass &q, uint32_t w, uint32_t slot) {
    return ((w & ((1u << (q.s0 - q.a)) - 1u)) << q.a) | (slot & ((1u << q.a) - 1u));
}
// the position in the column (in the order behind the bit-reversed load) of that slot: below 2^k
AESW_NTT_HD constexpr uint32_t ntt_slot_position(const NttPass &q, uint32_t w, uint32_t slot) {
    return ((w >> (q.s0 - q.a)) << (q.s0 + q.m)) | (ntt_slot_t(q, slot) << q.s0) | ntt_slot_lo(q, w, slot);
}
// the cell of the input column the first pass loads into a position
AESW_NTT_HD constexpr uint32_t ntt_first_source(uint32_t k, uint32_t position) { return ntt_bitrev(position, k); }
// what a later pass multiplies a slot's cell by as it loads it: omega_(2^(s0+m)) to this exponent (below 2^(s0+m)); 0 in the first pass
AESW_NTT_HD constexpr uint32_t ntt_slot_twiddle(const NttPass &q, uint32_t w, uint32_t slot) {
    return ntt_slot_lo(q, w, slot) * ntt_bitrev(ntt_slot_t(q, slot), q.m);
}
// butterfly b (below 2^(NTT_PASS_LOG - 1)) of stage j (1 ... m) of the pass: its lower slot; the upper one is `span` above it
AESW_NTT_HD constexpr uint32_t ntt_butterfly_span(const NttPass &q, uint32_t j) { return 1u << (j - 1u + q.a); }
AESW_NTT_HD constexpr uint32_t ntt_butterfly_slot(const NttPass &q, uint32_t j, uint32_t b) {
    const uint32_t g = j - 1u + q.a;
    return ((b >> g) << (g + 1u)) | (b & ((1u << g) - 1u));
}
// its twiddle as a cell of the short table: omega_(2^j)^(t mod 2^(j-1)) = omega_(2^NTT_PASS_LOG)^(that << (NTT_PASS_LOG - j))
AESW_NTT_HD constexpr uint32_t ntt_butterfly_twiddle(const NttPass &q, uint32_t j, uint32_t slot, bool inverse) {
    const uint32_t e = (ntt_slot_t(q, slot) & ((1u << (j - 1u)) - 1u)) << (NTT_PASS_LOG - j);
    return inverse ? (NTT_SLOTS - e) & (NTT_SLOTS - 1u) : e;
}
// omega_(2^log_order)^e as an exponent of omega_(2^max_k), or of its inverse: below 2^max_k
AESW_NTT_HD constexpr uint32_t ntt_root_exponent(uint32_t max_k, uint32_t log_order, uint32_t e, bool inverse) {
    const uint32_t big = e << (max_k - log_order);
    return inverse ? (0u - big) & ((1u << max_k) - 1u) : big;
}

// Where slot s lies in a limb's plane of LDS.  A cell is stored limb-planar -- limb i of slot s is word i * 2^NTT_PASS_LOG + index --
// so a lane moves one word at a time (32 banks, two groups of 32 lanes).  The 32 lanes of a group run 32 consecutive butterflies:
// at a span of 32 slots and more their slots are consecutive, one bank each; below it they are the 32 slots of a run of 64 whose
// bit g is clear, 16 residues twice.  Flipping the five low bits of every odd run of 32 sends the second half to the other 16.
AESW_NTT_HD constexpr uint32_t ntt_lds_index(uint32_t slot) { return NTT_PASS_LOG > 5 ? slot ^ ((0u - (slot >> 5 & 1u)) & 31u) : slot; }

// ---- the tables ---------------------------------------------------------------------------------------------------------------
// short: omega_(2^NTT_PASS_LOG)^j, j < 2^NTT_PASS_LOG; low: omega^j, j < 2^min(max_k, 14); high: omega^(j * 2^14), j < 2^max(max_k - 14, 0),
// omega = omega_(2^max_k) (4.21's split); scales: 2^-k * zeta0^v at cell 3 k + v for k <= 28, v < 3.
constexpr uint32_t NTT_SPLIT = SIGMA_SPLIT, NTT_SCALE_CELLS = 3u * (NTT_MAX_K + 1u);
AESW_NTT_HD constexpr uint32_t ntt_low_cells(uint32_t max_k) { return 1u << (max_k < NTT_SPLIT ? max_k : NTT_SPLIT); }
AESW_NTT_HD constexpr uint32_t ntt_high_cells(uint32_t max_k) { return max_k > NTT_SPLIT ? 1u << (max_k - NTT_SPLIT) : 1u; }
AESW_NTT_HD constexpr uint32_t ntt_low_index(uint32_t e) { return e & ((1u << NTT_SPLIT) - 1u); }
AESW_NTT_HD constexpr uint32_t ntt_high_index(uint32_t e) { return e >> NTT_SPLIT; }
AESW_NTT_HD constexpr uint32_t ntt_scale_index(uint32_t k, uint32_t v) { return 3u * k + v; }
struct NttTables {
    uint32_t short_at, low_at, high_at, scales_at, cells;  // in cells
};
AESW_NTT_HD constexpr NttTables ntt_tables(uint32_t max_k) {
    NttTables t{};
    t.short_at = 0;
    t.low_at = NTT_SLOTS;
    t.high_at = t.low_at + ntt_low_cells(max_k);
    t.scales_at = t.high_at + ntt_high_cells(max_k);
    t.cells = t.scales_at + NTT_SCALE_CELLS;
    return t;
}
AESW_NTT_HD constexpr uint64_t ntt_tables_bytes(uint32_t max_k) { return ntt_k_ok(max_k) ? (uint64_t)ntt_tables(max_k).cells * sizeof(Fr) : 0u; }
static_assert(ntt_tables_bytes(NTT_MAX_K) <= (2u << 20), "the tables of the largest transform stay within 2 MiB");
// cell `at` of the tables, as the tables kernel computes it
AESW_NTT_HD constexpr Fr ntt_table_cell(uint32_t max_k, uint32_t at) {
    const NttTables t = ntt_tables(max_k);
    if (at < t.low_at) return fr_pow_u32(sigma_omega(NTT_PASS_LOG), at);
    if (at < t.high_at) return fr_pow_u32(sigma_omega(max_k), at - t.low_at);
    if (at < t.scales_at) return fr_pow_u32(sigma_omega(max_k), (at - t.high_at) << NTT_SPLIT);  // < 2^max_k: no exponent wraps
    return fr_mul(fr_pow_u32(NTT_INV_TWO, (at - t.scales_at) / 3u), ntt_zeta0_power((at - t.scales_at) % 3u));
}

// ---- the workspace --------------------------------------------------------------------------------------------------------------
// One copy of the columns where a transform takes more than one pass: an in-place call's first pass permutes cells across
// workgroups and writes there.  A call whose output is not its input goes through its output and leaves the workspace alone.
AESW_NTT_HD constexpr uint64_t ntt_workspace_bytes(uint32_t k, uint32_t n_cols) {
    return ntt_shape_ok(k, n_cols) && ntt_passes(k) > 1 ? ntt_cells(k, n_cols) * sizeof(Fr) : 0u;
}

}  // namespace aesw
