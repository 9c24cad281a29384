// aesw_run.h -- a RUN of one circuit's blocks, [first_block, first_block + n_blocks), as the two accumulators count it
// (acc/aesw_acc.hip, vacc/aesw_vacc.hip): the run is cut at the set boundaries into PIECES, one per set it
// touches, and every piece into CHUNKS of `chunk` blocks; a pair of workgroups owns a chunk.  Stated once for the host, which
// plans the grid (run_plan), and for the kernels, which find their chunk in it (Run::chunk_at): both read run_piece.  No HIP call
// and no ROCm include: tests/test_run.py compiles this header alone with g++ and holds both against a walk over Placement::locate.
#pragma once
#include "aesw_placement.h"

namespace aesw {

// The default chunk, from the shape alone.  A pair of workgroups flushes up to 65 536 + 1 024 words however few
// blocks it counted, so a chunk is at least MIN_CHUNK blocks: 256 x 608 Xor lookups, more than twice the words of the flush,
// and 32 blocks per wave in front of a flush of 66 steps.  Above that the run is spread over TARGET_PAIRS pairs: the counters
// leave room for one workgroup per CU, and 128 pairs are 256 workgroups, one per CU of the chip.
constexpr uint64_t MIN_CHUNK = 256, TARGET_PAIRS = 128, MAX_PAIRS_PER_SET = 1ull << 22;
AESW_HD uint32_t run_default_chunk(uint64_t n_blocks) {
    const uint64_t spread = (n_blocks + TARGET_PAIRS - 1) / TARGET_PAIRS;  // n_blocks < 2^30: it fits
    return (uint32_t)(spread < MIN_CHUNK ? MIN_CHUNK : spread);
}

// The piece of the run [first, end) in `set`: the blocks [lo, hi), none (lo >= hi) where the run does not touch the set.
AESW_HD void run_piece(const Placement &place, uint64_t first, uint64_t end, uint32_t set, uint64_t &lo, uint64_t &hi) {
    const uint64_t s_lo = place.first_block(set), s_hi = s_lo + place.capacity(set);
    lo = first > s_lo ? first : s_lo;
    hi = end < s_hi ? end : s_hi;
}

// What workgroup (x, y) of the grid counts: the bins of `half` over blocks [b0, b0 + cnt) of `set`; cnt == 0: nothing.
struct RunChunk {
    uint32_t half, set;
    uint64_t b0, cnt;
};

// The run as a kernel's parameter struct embeds it, filled by run_plan.
struct Run {
    Placement place;
    uint64_t first, end;
    uint32_t set0;   // the set of block `first`: y counts the pieces from it
    uint32_t chunk;  // blocks per pair of workgroups
    AESW_HD RunChunk chunk_at(uint32_t x, uint32_t y) const {
        RunChunk c{x & 1u, set0 + y, 0, 0};
        uint64_t lo, hi;
        run_piece(place, first, end, c.set, lo, hi);
        c.b0 = lo + (uint64_t)(x >> 1) * chunk;
        if (c.b0 < hi) c.cnt = hi - c.b0 < chunk ? hi - c.b0 : chunk;  // fewer at the piece's end
        return c;
    }
};

// The host's plan of a run of n_blocks >= 1 blocks that the capacity holds (chunk 0: the default): a grid of (2 * pairs, pieces).
struct RunPlan {
    Run run;
    uint32_t pieces;         // the sets from the first block's to the last block's
    uint64_t longest, pairs;  // blocks of the longest piece, and its chunks
    AESW_HD bool fits() const { return pairs <= MAX_PAIRS_PER_SET; }
};
AESW_HD RunPlan run_plan(const Placement &place, uint64_t first_block, uint64_t n_blocks, uint32_t chunk) {
    RunPlan p{{place, first_block, first_block + n_blocks, 0, chunk ? chunk : run_default_chunk(n_blocks)}, 0, 0, 0};
    Run &r = p.run;
    uint32_t set1;
    uint64_t bi;
    place.locate<uint64_t>(r.first, r.set0, bi);
    place.locate<uint64_t>(r.end - 1, set1, bi);
    p.pieces = set1 - r.set0 + 1;
    // the longest of the first piece, the last, and one between them: every piece between the two is a whole set
    const uint32_t ends[3] = {r.set0, set1, p.pieces > 2 ? r.set0 + 1 : r.set0};
    for (const uint32_t s : ends) {
        uint64_t lo, hi;
        run_piece(place, r.first, r.end, s, lo, hi);
        if (hi - lo > p.longest) p.longest = hi - lo;
    }
    p.pairs = (p.longest + r.chunk - 1) / r.chunk;
    return p;
}

}  // namespace aesw
