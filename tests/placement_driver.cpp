// Drives the placement rule (csrc/aesw_placement.h, compiled alone: no ROCm include) -- tests/test_placement.py.
// Commands on stdin, one answer line each:
//   c <k>               "<cap0> <capn>"
//   b <k> <n_sets> <j>  "<total> -" when block j is past the capacity `total` of n_sets sets, else "<total> <set> <row> <set32> <row32>":
//                       block j's place through the 64-bit division and through the 32-bit one (k <= 30; "- -" above)
//   f <k> <n_sets> <n>  the blocks of every set that a circuit of n blocks fills, and each set's first block and first row:
//                       n_sets x "<filled>:<first_block>:<first_row>"
#include "aesw_placement.h"

#include <cinttypes>
#include <cstdio>

int main() {
    char cmd;
    uint32_t k, n_sets;
    uint64_t j;
    while (std::scanf(" %c %" SCNu32, &cmd, &k) == 2) {
        const aesw::Placement pl(k);
        if (cmd == 'c') {
            std::printf("%" PRIu64 " %" PRIu64 "\n", pl.cap0, pl.capn);
            continue;
        }
        if (std::scanf("%" SCNu32 " %" SCNu64, &n_sets, &j) != 2) return 2;
        if (cmd == 'b') {
            const uint64_t total = pl.total(n_sets);
            if (j >= total) {
                std::printf("%" PRIu64 " -\n", total);
                continue;
            }
            uint32_t set, set32 = 0, bi32 = 0;
            uint64_t bi;
            pl.locate(j, set, bi);
            std::printf("%" PRIu64 " %" PRIu32 " %" PRIu64, total, set, aesw::Placement::row_of(set, bi));
            if (k <= 30) {
                pl.locate(j, set32, bi32);
                std::printf(" %" PRIu32 " %" PRIu64 "\n", set32, aesw::Placement::row_of(set32, bi32));
            } else {
                std::printf(" - -\n");
            }
        } else if (cmd == 'f') {
            for (uint32_t s = 0; s < n_sets; ++s)
                std::printf("%s%" PRIu64 ":%" PRIu64 ":%" PRIu32, s ? " " : "", pl.filled(s, j), pl.first_block(s), aesw::Placement::first_row(s));
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
