// The arrangement rule of csrc/aesw_perm.h run on the CPU, for tests/test_perm_model.py: the header compiled alone with g++.
//   perm_rule_driver HIST OUT TAG U PAD [U PAD ...]
// HIST: one histogram, 66 561 little-endian uint32.  Per (U, PAD): perm_scan_host over a poisoned workspace, then perm_cell for
// every position; A' and S' (U uint32 each) are appended to OUT and the argument's four scalars printed on a line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aesw_perm.h"

int main(int argc, char **argv) {
    using namespace aesw;
    if (argc < 6 || (argc - 4) % 2) return 2;
    std::vector<uint32_t> hist(MULT_BINS);
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out || std::fread(hist.data(), 4, MULT_BINS, in) != MULT_BINS) return 3;
    const uint32_t tag = (uint32_t)std::atoi(argv[3]);
    for (int i = 4; i < argc; i += 2) {
        const uint32_t u = (uint32_t)std::strtoul(argv[i], nullptr, 10), pad = (uint32_t)std::strtoul(argv[i + 1], nullptr, 10);
        if (!perm_k_ok(17) || !perm_rows_ok(17, u) || pad >= MULT_BINS) return 4;
        std::vector<uint32_t> ws(PERM_WS_WORDS, 0xdeadbeefu), a(u), s(u);
        perm_scan_host(hist.data(), tag, u, ws.data());
        const PermArgument arg = perm_argument(ws.data(), tag, u, pad);
        for (uint32_t p = 0; p < u; ++p) {
            const PermCell c = perm_cell(arg, p);
            a[p] = c.a;
            s[p] = c.s;
        }
        if (std::fwrite(a.data(), 4, u, out) != u || std::fwrite(s.data(), 4, u, out) != u) return 5;
        std::printf("%u %u %u %u\n", arg.sc.z, arg.sc.d, arg.sc.zero_used, arg.sc.overflow);
    }
    std::fclose(out);
    return 0;
}
