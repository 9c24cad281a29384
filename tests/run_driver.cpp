// Drives the run of one circuit's blocks (csrc/aesw_run.h, compiled alone: no ROCm include) -- tests/test_run.py.
// Commands on stdin, one answer line each:
//   d <n_blocks>                            "<run_default_chunk(n_blocks)>"
//   p <k> <n_sets> <first> <n> <chunk>      "<set0> <pieces> <longest> <pairs> <chunk> <fits>" of run_plan (chunk 0: the default)
//   s <k> <n_sets>                          the sweep: every (first, n >= 1) with first + n <= capacity, under chunks 1, 2, 5, 17 and
//                                           the default.  The plan against a count that places every block of the run with
//                                           Placement::locate; Run::chunk_at at every (x, y) of the planned grid: its chunks lie in
//                                           their set and in the run and cover each block of the run once per half.
//                                           "<capacity> <cases> <failures>", and on stderr the first failure
#include "aesw_run.h"

#include <cinttypes>
#include <cstdio>
#include <vector>

using namespace aesw;

static const char *check(const Placement &pl, uint32_t n_sets, uint64_t first, uint64_t n, uint32_t chunk) {
    const RunPlan plan = run_plan(pl, first, n, chunk);
    const Run &r = plan.run;
    // by brute force: the blocks of the run in every set
    std::vector<uint64_t> in_set(n_sets, 0);
    for (uint64_t j = first; j < first + n; ++j) {
        uint32_t set;
        uint64_t bi;
        pl.locate(j, set, bi);
        if (set >= n_sets) return "locate() leaves the circuit";
        ++in_set[set];
    }
    uint32_t lo = 0, hi = n_sets - 1;
    while (in_set[lo] == 0) ++lo;
    while (in_set[hi] == 0) --hi;
    uint64_t longest = 0;
    for (uint32_t s = lo; s <= hi; ++s) longest = in_set[s] > longest ? in_set[s] : longest;
    const uint64_t want_chunk = chunk ? chunk : run_default_chunk(n);
    if (r.first != first || r.end != first + n || r.chunk != want_chunk || r.place.cap0 != pl.cap0 || r.place.capn != pl.capn) return "the run's fields";
    if (r.set0 != lo) return "set0";
    if (plan.pieces != hi - lo + 1) return "pieces";
    if (plan.longest != longest) return "longest";
    if (plan.pairs != (longest + want_chunk - 1) / want_chunk || !plan.fits()) return "pairs";
    // the kernels' side, over the planned grid
    std::vector<uint32_t> seen[2] = {std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0)};
    for (uint32_t y = 0; y < plan.pieces; ++y)
        for (uint64_t x = 0; x < 2 * plan.pairs; ++x) {
            const RunChunk c = r.chunk_at((uint32_t)x, y);
            if (c.half != (x & 1) || c.set != lo + y) return "half or set of a workgroup";
            if (c.cnt > want_chunk) return "a chunk longer than `chunk`";
            for (uint64_t b = c.b0; b < c.b0 + c.cnt; ++b) {
                if (b < first || b >= first + n) return "a chunk outside the run";
                uint32_t set;
                uint64_t bi;
                pl.locate(b, set, bi);
                if (set != c.set) return "a chunk across a set boundary";
                ++seen[c.half][b - first];
            }
        }
    for (uint64_t i = 0; i < n; ++i)
        if (seen[0][i] != 1 || seen[1][i] != 1) return "a block not covered once per half";
    return nullptr;
}

int main() {
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        if (cmd == 'd') {
            uint64_t n;
            if (std::scanf("%" SCNu64, &n) != 1) return 2;
            std::printf("%" PRIu32 "\n", run_default_chunk(n));
            continue;
        }
        uint32_t k, n_sets;
        if (std::scanf("%" SCNu32 " %" SCNu32, &k, &n_sets) != 2) return 2;
        const Placement pl(k);
        if (cmd == 'p') {
            uint64_t first, n;
            uint32_t chunk;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu32, &first, &n, &chunk) != 3) return 2;
            const RunPlan plan = run_plan(pl, first, n, chunk);
            std::printf("%" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu32 " %d\n", plan.run.set0, plan.pieces, plan.longest, plan.pairs, plan.run.chunk,
                        (int)plan.fits());
        } else if (cmd == 's') {
            const uint64_t cap = pl.total(n_sets);
            uint64_t cases = 0, failures = 0;
            for (uint64_t first = 0; first < cap; ++first)
                for (uint64_t n = 1; first + n <= cap; ++n)
                    for (const uint32_t chunk : {1u, 2u, 5u, 17u, 0u}) {
                        ++cases;
                        if (const char *why = check(pl, n_sets, first, n, chunk)) {
                            if (failures++ == 0)
                                std::fprintf(stderr, "k %" PRIu32 " n_sets %" PRIu32 " first %" PRIu64 " n %" PRIu64 " chunk %" PRIu32 ": %s\n", k, n_sets, first, n,
                                             chunk, why);
                        }
                    }
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", cap, cases, failures);
        } else {
            return 2;
        }
    }
    return 0;
}
