// aesw_open.h -- the rules of libaesw_open.so, once: a coefficient column at a point.  With
//   S_n = 0,  S_i = c_i + z * S_(i+1)                                                                  (the serial recurrence)
// the value of the column's polynomial is p(z) = S_0 and the quotient (p(X) - p(z)) / (X - z) has the coefficients q[i] = S_(i+1):
// evaluation and division are one suffix recurrence, additive and weighted by powers of z.  Here: the bounds, how the 2^k cells of
// a column are cut into the chunks the passes of open/aesw_open.hip share, which power z^(2^s) joins which two pieces, the
// workspace, the fold of columns under v, and the recurrence itself -- written once for the kernels and for the CPU driver of
// tests/open_driver.cpp.  The field is aesw_fr.h's; nothing of it is restated.
// No HIP call and no ROCm include: tests/test_open_model.py compiles this header alone with g++.
//
// The value V of a piece c_a ... c_(b-1) is sum c_i z^(i-a); a piece in front of another joins it as
//   V(front ++ behind) = V(front) + z^len(front) * V(behind)                                           (open_join)
// and every piece the passes join has a length 2^s, so the only powers needed are z^(2^s):
//   a lane      OPEN_ROWS_PER_LANE = 4 consecutive cells by Horner, from the top                       z             (s = 0)
//   a wave      the suffix scan over its 64 lanes, step o = 1, 2 ... 32 joins pieces of 4 o cells     z^(4 o)       (s = 2 ... 7)
//   a workgroup its 4 waves of 256 cells each by Horner, from the top                                  z^256         (s = 8)
//   a column    the suffix scan over its chunks of 1 024 cells, step o joins pieces of 1 024 o         z^(1024 o)    (s = 10 ... 15),
//               the waves of a turn of 256 chunks (2^16 cells each)                                    z^65536       (s = 16)
//               and one turn hands the value of everything above it to the next, as the cell behind its top lane.
// What lies ABOVE a lane's piece enters by the lane's own weight z^(unit * (64 - lane)) (open_lane_weight): the top lane is one
// unit below the wave's end.  z = 0 takes the same path: every power is 0 and every join returns its front.
#pragma once
#include <stdint.h>

#include "aesw_fr.h"

#if defined(__HIPCC__)
#define AESW_OPEN_ROLLED _Pragma("unroll 1")  // a loop that stays a loop: it indexes no array of cells, and its body is a product of code
#else
#define AESW_OPEN_ROLLED
#endif

namespace aesw {

constexpr uint32_t OPEN_ROWS_PER_LANE = 4;  // consecutive cells of a column a lane of the chunk and scan kernels owns: one 128-byte read
constexpr uint32_t OPEN_LANES = 64;
constexpr uint32_t OPEN_THREADS = 256, OPEN_WAVES = OPEN_THREADS / OPEN_LANES, OPEN_CHUNK = OPEN_THREADS * OPEN_ROWS_PER_LANE;  // cells of one workgroup
constexpr uint32_t OPEN_TURN = OPEN_THREADS;  // chunks the carry kernel scans at a time
constexpr uint32_t OPEN_MIN_K = 10, OPEN_MAX_K = 28, OPEN_MAX_COLS = 65535, OPEN_MAX_POINTS = 16;
constexpr uint32_t OPEN_POWERS = OPEN_MAX_K + 1;  // z^(2^s), s = 0 ... 28, per point
static_assert(OPEN_ROWS_PER_LANE == 4 && OPEN_CHUNK == 1024, "the power indices below are those of four cells a lane");
static_assert(OPEN_CHUNK == 1u << OPEN_MIN_K, "the smallest column is one chunk: every column is whole chunks");

constexpr bool open_k_ok(uint32_t k) { return k >= OPEN_MIN_K && k <= OPEN_MAX_K; }
constexpr bool open_cols_ok(uint32_t n_cols) { return n_cols >= 1 && n_cols <= OPEN_MAX_COLS; }
constexpr bool open_points_ok(uint32_t n_points) { return n_points >= 1 && n_points <= OPEN_MAX_POINTS; }

// ---- the chunks and the turns ------------------------------------------------------------------------------------------------
constexpr uint32_t open_chunks(uint32_t k) { return (1u << k) / OPEN_CHUNK; }  // of one column; a power of two, 1 ... 2^18
constexpr uint32_t open_turns(uint32_t k) { return (open_chunks(k) + OPEN_TURN - 1) / OPEN_TURN; }
// the first chunk of turn t: the turns go from the last chunk down; a column of fewer chunks than a turn has one turn from 0
constexpr uint32_t open_turn_first(uint32_t k, uint32_t t) { return (open_turns(k) - 1 - t) * OPEN_TURN; }
static_assert(open_turns(18) == 1 && open_turns(19) == 2 && open_turn_first(19, 0) == 256 && open_turn_first(19, 1) == 0 && open_turns(28) == 1024,
              "k = 19 is the smallest column whose carry takes a second turn");

// ---- the powers: cell s of a point is z^(2^s) --------------------------------------------------------------------------------
constexpr uint32_t OPEN_POWER_CELL = 0;        // z: a lane's Horner
constexpr uint32_t OPEN_POWER_LANE = 2;        // z^4: a lane's piece; the wave scan's step o = 2^j takes OPEN_POWER_LANE + j
constexpr uint32_t OPEN_POWER_WAVE = 8;        // z^256: a wave's piece
constexpr uint32_t OPEN_POWER_CHUNK = 10;      // z^1024: a chunk; the carry's wave scan takes OPEN_POWER_CHUNK + j
constexpr uint32_t OPEN_POWER_CHUNK_WAVE = 16; // z^65536: the 64 chunks of a wave of the carry kernel
constexpr uint32_t open_scan_power(uint32_t base, uint32_t j) { return base + j; }  // of the step o = 2^j, j = 0 ... 5
static_assert(OPEN_POWER_LANE + 6 == OPEN_POWER_WAVE && OPEN_POWER_WAVE + 2 == OPEN_POWER_CHUNK && OPEN_POWER_CHUNK + 6 == OPEN_POWER_CHUNK_WAVE &&
                  OPEN_POWER_CHUNK_WAVE < OPEN_POWERS,
              "4 * 64 = 256 cells a wave, 4 waves a chunk, 64 chunks a wave of the carry");

// ---- the workspace: the powers of every point, then one cell per chunk, column and point -------------------------------------
constexpr uint64_t open_power_at(uint32_t point, uint32_t s) { return (uint64_t)point * OPEN_POWERS + s; }
constexpr uint64_t open_chunk_cells_at(uint32_t n_points) { return (uint64_t)n_points * OPEN_POWERS; }  // where the chunk cells begin
// the chunk cells of (column, point): open_chunks(k) cells, one behind the other
constexpr uint64_t open_chunk_at(uint32_t k, uint32_t n_points, uint32_t column, uint32_t point, uint32_t chunk) {
    return open_chunk_cells_at(n_points) + ((uint64_t)column * n_points + point) * open_chunks(k) + chunk;
}
constexpr uint64_t open_workspace_cells(uint32_t k, uint32_t n_cols, uint32_t n_points) { return open_chunk_at(k, n_points, n_cols, 0, 0); }
constexpr uint64_t open_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t n_points) {
    return open_k_ok(k) && open_cols_ok(n_cols) && open_points_ok(n_points) ? open_workspace_cells(k, n_cols, n_points) * sizeof(Fr) : 0u;
}
static_assert(open_workspace_bytes(10, 1, 1) == 30 * 32 && open_workspace_bytes(28, 65535, 16) == ((uint64_t)16 * 29 + (uint64_t)65535 * 16 * (1u << 18)) * 32 &&
                  open_workspace_bytes(9, 1, 1) == 0 && open_workspace_bytes(10, 1, 17) == 0,
              "the workspace: 29 powers a point and one cell per chunk, column and point; 0 outside the bounds");

// ---- the recurrence ----------------------------------------------------------------------------------------------------------

// front + weight * behind: the value of a piece and the piece behind it, weight = z^len(front)
AESW_MONT_HD constexpr Fr open_join(const Fr &front, const Fr &weight, const Fr &behind) { return fr_add(front, fr_mul(weight, behind)); }

// The serial recurrence over n cells from the top, S_n = above: s(i, S_i) for i = n - 1 ... 0; returns S_0.  What the passes compute
// piecewise, and what tests/open_driver.cpp holds them against.
template <class Load, class Out>
AESW_MONT_HD Fr open_serial(uint64_t n, const Fr &z, const Fr &above, Load &&load, Out &&s) {
    Fr acc = above;
    for (uint64_t i = n; i-- > 0;) {
        acc = open_join(load(i), z, acc);
        s(i, acc);
    }
    return acc;
}

// A lane's cells c[0 ... 3] from the top by Horner: h[q] = S at the lane's cell q with nothing above the lane; h[0] is the value
// of the lane's piece.  Three products.
AESW_MONT_HD void open_lane_horner(const Fr (&c)[OPEN_ROWS_PER_LANE], const Fr &z, Fr (&h)[OPEN_ROWS_PER_LANE]) {
    h[OPEN_ROWS_PER_LANE - 1] = c[OPEN_ROWS_PER_LANE - 1];
    fr_unrolled<OPEN_ROWS_PER_LANE - 1>([&](auto at) {
        constexpr int q = OPEN_ROWS_PER_LANE - 2 - decltype(at)::value;
        h[q] = open_join(c[q], z, h[q + 1]);
    });
}

// The quotient's cells of a lane: above = S at the cell behind the lane's last; q[j] = S at the lane's cell j + 1.  Three products.
AESW_MONT_HD void open_lane_quotient(const Fr (&c)[OPEN_ROWS_PER_LANE], const Fr &z, const Fr &above, Fr (&q)[OPEN_ROWS_PER_LANE]) {
    q[OPEN_ROWS_PER_LANE - 1] = above;
    fr_unrolled<OPEN_ROWS_PER_LANE - 1>([&](auto at) {
        constexpr int j = OPEN_ROWS_PER_LANE - 2 - decltype(at)::value;
        q[j] = open_join(c[j + 1], z, q[j + 1]);
    });
}

// z^(unit * (64 - lane)) from the powers power(s) = z^(2^s), unit = 2^base: what multiplies the value above a wave in lane
// `lane`, whose piece begins 64 - lane units below the wave's end.  64 - lane is 1 ... 64: seven bits, a product for every one.
template <class Power>
AESW_MONT_HD Fr open_lane_weight(uint32_t base, uint32_t lane, Power &&power) {
    const uint32_t e = OPEN_LANES - lane;
    Fr w = FR_ONE;
    AESW_OPEN_ROLLED
    for (uint32_t b = 0; b < 7; ++b) {
        const Fr m = fr_mul(w, power(base + b));
        if (e >> b & 1u) w = m;
    }
    return w;
}

// The waves of a workgroup, or of a turn, from the top: total(w) the value of wave w's piece, weight = z^len(a wave's piece),
// `above` what lies above the last wave.  above_of(w, value) is told the value above wave w; returns the value of everything
// from wave 0 up.  (Callables, not arrays: a kernel keeps the one value of its own wave.)
template <int WAVES, class Total, class Above>
AESW_MONT_HD Fr open_join_waves(const Fr &weight, const Fr &above, Total &&total, Above &&above_of) {
    Fr acc = above;
    fr_unrolled<WAVES>([&](auto at) {
        constexpr int w = WAVES - 1 - decltype(at)::value;
        above_of(w, acc);
        acc = open_join(total(w), weight, acc);
    });
    return acc;
}

// ---- the fold of columns under v -----------------------------------------------------------------------------------------------
// acc = acc * v + col, column after column: (...((acc * v + col_0) * v + col_1)...) * v + col_(n-1) -- the order of halo2 v0.3.0's
// GWC prover as remembered, not pinned by a test.
AESW_MONT_HD constexpr Fr open_fold_step(const Fr &acc, const Fr &v, const Fr &col) { return fr_add(fr_mul(acc, v), col); }

}  // namespace aesw
