// aesw_flush.h -- the whole-line flush of the staging windows (aesw_layout.h Win<>): its closed-form specification, the
// table-driven "scheduled flush" the kernel runs, the LDS bank model and the quad search that orders a round's lines.
// Shared by the encrypt kernels (aesw_kernels.hip) and the host-side lane model of the tests; nothing that only reads or
// checks slabs needs it.
#pragma once
#include "aesw_layout.h"

namespace aesw {

// Whole-line flush after round R (1..9; flush 9 also carries round 10).
// For block b of a wave (column bytes [b*GSTRIDE, (b+1)*GSTRIDE) of the wave's
// line-aligned 16-block range) the lines that just became complete are
// [lo, hi); piece (t, sub) is 16 bytes of line lo+t.  Returns where the piece
// sits in the wave's LDS column stage (block windows of W::BYTES) and where it
// goes in the wave's global range.  This closed form is the SPECIFICATION (when a line leaves, from which LDS
// bytes); the kernel runs the table-driven "scheduled flush" below, which the tests check against it.
struct FlushPiece {
    bool ok;
    int lds_off;  // relative to the wave's stage of this column
    int P;        // byte offset in the wave's 16-block column range
};

template <class W>
AESW_HD constexpr int flush_maxc(int R) {
    return ((R == 1 ? W::end(1) : W::end(R == 9 ? 10 : R) - W::end(R - 1)) + 127) / 128 + (R == 9 ? 1 : 0);
}

template <class W>
AESW_HD FlushPiece flush_piece(int R, int b, int sub, int t, int nvalid) {
    const int rmin = R - (W::NSLOT - 1) < 1 ? 1 : R - (W::NSLOT - 1);
    const int base = b * W::GSTRIDE;
    // Block b's own rounds never flush the line that holds the previous block's tail: it leaves with that
    // block's last flush.  While head + rounds stay short of the first line boundary (z, values-only y) the
    // lower bound is therefore the first line that STARTS inside the block, not the line base falls into.
    const int first = (base + 127) >> 7;
    const int lo_raw = R == 1 ? first : (base + W::end(R - 1)) >> 7;
    const int lo = lo_raw < first ? first : lo_raw;
    const int hi = R == 9 ? (base + W::GSTRIDE + 127) >> 7 : (base + W::end(R)) >> 7;
    const int k = lo + t;
    const int P = 128 * k + 16 * sub;
    int o = P - base;  // block-relative offset of this piece
    bool ok = k < hi && b < nvalid;
    int a = b * W::BYTES;
    int adj = W::woff(rmin) - W::start(rmin);  // window offset = o + adj
    for (int r = rmin + 1; r <= R; ++r) adj = o >= W::start(r) ? W::woff(r) - W::start(r) : adj;
    if (R == 9) {
        adj = o >= W::start(10) ? W::woff(10) - W::start(10) : adj;
        if (o >= W::GSTRIDE) {
            // the tail of this line is the next block's head, which its window kept
            ok = ok && b + 1 < nvalid;
            a += W::BYTES;
            o -= W::GSTRIDE;
            adj = 0;
        }
    }
    return FlushPiece{ok, a + o + adj, P};
}

// ---- scheduled flush (round 2) ---------------------------------------------------------------------------
// The set of 128-byte lines of a wave's 16-block column range that complete in round R is the same for every full
// wave: it only depends on the column geometry.  So the flush is a fixed schedule instead of per-round address
// arithmetic: the lines of round R in address order, eight per store instruction (lane = (line slot lane>>3, 16-byte
// piece lane&7)), and for every (instruction, lane) ONE descriptor word that says where the piece sits in the wave's
// LDS stage and where it goes in the wave's global range.  The kernel loads its descriptors once (one dword per
// lane and instruction, from a table the host builds with build_flush_table()) and keeps them in registers; a piece
// then costs two VALU instructions instead of ~12, and ~55 instead of ~90 store instructions leave per wave.
// flush_piece() above remains the specification of WHEN a line leaves and where its bytes are staged; the tests
// check that the schedule stores every piece exactly once from the same LDS bytes.
//   descriptor = lds_off | P << 16      lds_off: byte offset in the column's wave stage (the kernel adds the stage base;
//                                        the sum must stay below 64 KiB), P: byte offset in the wave's global range;
//   an unused slot has P = SCHED_INVALID_P (above any range), so "P < nvalid*GSTRIDE" is the store predicate of a
//   partial wave and of a partial instruction alike.
constexpr int SCHED_BPW = 16;
constexpr uint32_t SCHED_INVALID_P = 0x7ff0u;

// the round (1..9) whose flush carries block-relative byte o: the head leaves with round 1, round 10 with round 9
template <class W>
AESW_HD constexpr int sched_round_of(int o) {
    for (int R = 1; R <= 8; ++R)
        if (o < W::end(R)) return R;
    return 9;
}
// the round in which line k of the wave's range is complete
template <class W>
AESW_HD constexpr int sched_line_round(int k) {
    int r = 1;
    for (int s = 0; s < 8; ++s) {
        const int P = 128 * k + 16 * s, b = P / W::GSTRIDE, o = P - b * W::GSTRIDE;
        const int q = sched_round_of<W>(o);
        r = q > r ? q : r;
    }
    return r;
}
template <class W>
AESW_HD constexpr int sched_nlines(int R) {
    int n = 0;
    for (int k = 0; k < SCHED_BPW * W::GSTRIDE / 128; ++k) n += sched_line_round<W>(k) == R ? 1 : 0;
    return n;
}
template <class W> AESW_HD constexpr int sched_ninstr(int R) { return (sched_nlines<W>(R) + 7) / 8; }
// index of round R's first instruction in the column's descriptor list; sched_first(10) = their total number
template <class W>
AESW_HD constexpr int sched_first(int R) {
    int n = 0;
    for (int r = 1; r < R; ++r) n += sched_ninstr<W>(r);
    return n;
}
// where block-relative byte o is staged inside the block's window
template <class W>
AESW_HD constexpr int sched_window_offset(int o) {
    if (o < W::HEAD) return o;
    const int r = o >= W::start(10) ? 10 : (o - W::HEAD) / W::ROUND + 1;
    return W::woff(r) + (o - W::start(r));
}
// LDS bank cost of one ds_read_b128 whose lane l reads 16 bytes at addr[l] (addr < 0: lane idle).  gfx950 serves the
// instruction in four passes of 16 lanes -- {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32 -- over 64 banks
// of 4 bytes (MI355X_MICROARCH.md, LDS); a pass needs as many cycles as its busiest bank has distinct dwords.
inline int b128_read_conflict_cost(const int addr[64]) {
    static const int pass_lanes[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                          {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    int cost = 0;
    for (int half = 0; half < 2; ++half)
        for (int p = 0; p < 2; ++p) {
            int load[64] = {0};
            int worst = 1;
            for (int i = 0; i < 16; ++i) {
                const int a = addr[pass_lanes[p][i] + 32 * half];
                if (a < 0) continue;
                for (int d = 0; d < 4; ++d) {
                    const int bank = ((a >> 2) + d) & 63;
                    if (++load[bank] > worst) worst = load[bank];
                }
            }
            cost += worst - 1;
        }
    return cost;
}

// Pure host: the column's whole table, sched_first<W>(10) * 64 words, instruction-major (word i*64 + lane).
// Which line takes which slot of its round's instructions does not matter to the global stores (every slot is one
// whole line); it matters to the LDS: the eight lines of an instruction are gathered by ONE ds_read_b128, and line
// starts that collide in the banks cost cycles (PMC, round 2: 58 % of the flush's LDS-active cycles were bank
// conflicts with the lines in address order; this model reproduces the measured 308 conflict cycles per wave as 304).
// The four passes of a ds_read_b128 pair up slots 0-3 and slots 4-7 independently, so a round's lines are dealt into
// QUADS: greedily the cheapest quad that contains the first line still free (its three partners and the split into the
// slot pairs {0,3} / {1,2} by exhaustive search), then pairwise swaps between slots while the summed cost drops.
// Deterministic; ~20 ms per layout.  Unused slots all fall into the round's last instruction.
template <class W>
inline void build_flush_table(uint32_t *out) {
    // the descriptor packs a 16-bit LDS offset below P: every valid P must lie below the "unused slot" sentinel, and a
    // wave's stage of this column must be addressable with 16 bits (the kernel adds the stage base: launch_enc checks the sum)
    static_assert((uint32_t)(SCHED_BPW * W::GSTRIDE) <= SCHED_INVALID_P, "a wave's global range of this column reaches the unused-slot sentinel");
    static_assert(SCHED_BPW * W::BYTES <= 65536, "a wave's LDS stage of this column needs more than 16 address bits");
    static_assert(SCHED_INVALID_P < 0x8000u, "P << 16 must fit the descriptor word's upper half");
    constexpr int NL = SCHED_BPW * W::GSTRIDE / 128;
    int line_round[NL];
    for (int k = 0; k < NL; ++k) line_round[k] = sched_line_round<W>(k);
    auto piece = [](int line, int sub, int *lds, int *P) {
        *P = 128 * line + 16 * sub;
        const int b = *P / W::GSTRIDE, o = *P - b * W::GSTRIDE;
        *lds = b * W::BYTES + sched_window_offset<W>(o);
    };
    auto quad_cost = [&](const int q[4]) {  // four line slots = lanes 0..31 of one instruction; -1 = unused slot
        int addr[64];
        for (int l = 0; l < 64; ++l) addr[l] = -1;
        for (int sl = 0; sl < 4; ++sl)
            if (q[sl] >= 0)
                for (int sub = 0; sub < 8; ++sub) {
                    int P;
                    piece(q[sl], sub, &addr[8 * sl + sub], &P);
                }
        return b128_read_conflict_cost(addr);
    };
    auto best_split = [&](const int m[4], int q[4]) {  // the three ways to pair four members onto slots {0,3} and {1,2}
        static const int pairings[3][4] = {{0, 1, 2, 3}, {0, 2, 1, 3}, {0, 3, 1, 2}};
        int best = 1 << 30;
        for (const auto &p : pairings) {
            const int t[4] = {m[p[0]], m[p[2]], m[p[3]], m[p[1]]};
            const int c = quad_cost(t);
            if (c < best) {
                best = c;
                for (int i = 0; i < 4; ++i) q[i] = t[i];
            }
        }
        return best;
    };
    int idx = 0;
    for (int R = 1; R <= 9; ++R) {
        int lines[NL], n = 0;
        for (int k = 0; k < NL; ++k)
            if (line_round[k] == R) lines[n++] = k;
        const int ni = (n + 7) / 8;
        int slots[NL + 8];  // the round's line slots, instruction-major; -1 = unused
        for (int i = 0; i < 8 * ni; ++i) slots[i] = -1;
        bool used[NL] = {false};
        int left = n, nq = 0;
        while (left > 0) {
            int f = 0;
            while (used[f]) ++f;
            int best = 1 << 30, pick[4] = {f, -1, -1, -1}, q[4], bq[4] = {lines[f], -1, -1, -1};
            if (left >= 4) {
                for (int a = f + 1; a < n; ++a) {
                    if (used[a]) continue;
                    for (int b = a + 1; b < n; ++b) {
                        if (used[b]) continue;
                        for (int c = b + 1; c < n; ++c) {
                            if (used[c]) continue;
                            const int m[4] = {lines[f], lines[a], lines[b], lines[c]};
                            const int cost = best_split(m, q);
                            if (cost < best) {
                                best = cost;
                                pick[1] = a; pick[2] = b; pick[3] = c;
                                for (int i = 0; i < 4; ++i) bq[i] = q[i];
                            }
                        }
                    }
                }
            } else {  // the last, partial quad: everything that is left
                int m[4] = {-1, -1, -1, -1}, j = 0;
                for (int i = 0; i < n; ++i)
                    if (!used[i]) { m[j] = lines[i]; pick[j] = i; ++j; }
                best_split(m, bq);
            }
            for (int i = 0; i < 4; ++i) {
                if (pick[i] >= 0) { used[pick[i]] = true; --left; }
                slots[4 * nq + i] = bq[i];
            }
            ++nq;
        }
        // refinement: swap two slots (of different quads, or re-pair inside one) while the summed cost drops
        auto cost_of = [&](int quad) { return quad_cost(slots + 4 * quad); };
        const int first_free_instr = (n / 8);  // instructions before this one are full: keep unused slots out of them
        for (bool improved = true; improved;) {
            improved = false;
            for (int s0 = 0; s0 < 8 * ni; ++s0)
                for (int s1 = s0 + 1; s1 < 8 * ni; ++s1) {
                    if (slots[s0] < 0 && slots[s1] < 0) continue;
                    if ((slots[s0] < 0 || slots[s1] < 0) && (s0 / 8 < first_free_instr || s1 / 8 < first_free_instr)) continue;
                    const int q0 = s0 / 4, q1 = s1 / 4;
                    const int before = cost_of(q0) + (q1 != q0 ? cost_of(q1) : 0);
                    if (before == 0) continue;
                    const int t = slots[s0]; slots[s0] = slots[s1]; slots[s1] = t;
                    const int after = cost_of(q0) + (q1 != q0 ? cost_of(q1) : 0);
                    if (after < before) improved = true;
                    else { slots[s1] = slots[s0]; slots[s0] = t; }
                }
        }
        for (int i = 0; i < ni; ++i, ++idx)
            for (int lane = 0; lane < 64; ++lane) {
                const int line = slots[8 * i + (lane >> 3)];
                uint32_t d = SCHED_INVALID_P << 16;  // unused slots: only in the round's last instruction
                if (line >= 0) {
                    int lds, P;
                    piece(line, lane & 7, &lds, &P);
                    d = (uint32_t)lds | ((uint32_t)P << 16);
                }
                out[idx * 64 + lane] = d;
            }
    }
}

// Summed b128_read_conflict_cost of a column's table (tests, tools): extra LDS cycles per wave.
template <class W>
inline int flush_table_conflict_cost(const uint32_t *tab) {
    int cost = 0;
    for (int i = 0; i < sched_first<W>(10); ++i) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t d = tab[i * 64 + lane];
            addr[lane] = (d >> 16) == SCHED_INVALID_P ? -1 : (int)(d & 0xffffu);
        }
        cost += b128_read_conflict_cost(addr);
    }
    return cost;
}

}  // namespace aesw
