// tests/test_mult_rule.py: csrc/aesw_mult.h compiled alone (no ROCm include), answering on stdin / stdout.
//   first line:  768 table bytes (sbox | mul2 | mul3) as decimals
//   "r t x y z": one (tag, x, y, z)                       -> "bin hit"
//   "m t":       every (x, y) of a one-operand tag 3..5   -> the number of hits, and of hits whose bin is not first + x
//   "x s":       the Xor tag, every (x, y) with z = x ^ y and with z = x ^ y ^ (1 + (x * 31 + y + s) % 255)
//                -> hits of the first kind whose bin is 512 + 256 x + y, hits of the second kind
//   "s":         the counter split over every tag 1..5 and every (x, y), and the flush ranges of both halves
//                -> lookups owned by exactly one half; owners' counters at or past MULT_COUNTERS; pairs of different bins of one
//                   half on one counter; bins 0 .. 66 559 the ranges cover exactly once; times a range reaches the zero row or
//                   leaves the counters; counters a range maps to another bin than the index rule sent there
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "aesw_mult.h"

int main() {
    uint8_t tab[768];
    for (int i = 0; i < 768; ++i) { int v; std::cin >> v; tab[i] = (uint8_t)v; }
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "r") {
            uint32_t t, x, y, z;
            std::cin >> t >> x >> y >> z;
            std::printf("%u %d\n", aesw::mult_bin(t, x, y), (int)aesw::mult_hit(t, x, y, z, tab));
        } else if (cmd == "m") {
            uint32_t t;
            std::cin >> t;
            unsigned hits = 0, wrong = 0;
            for (uint32_t x = 0; x < 256; ++x)
                for (uint32_t y = 0; y < 256; ++y)
                    for (uint32_t z = 0; z < 256; z += 85)  // z is ignored
                        if (aesw::mult_hit(t, x, y, z, tab)) {
                            ++hits;
                            wrong += y != tab[(t - 3) * 256 + x] || aesw::mult_bin(t, x, y) != aesw::mult_section_first(t) + x;
                        }
            std::printf("%u %u\n", hits, wrong);
        } else if (cmd == "x") {
            uint32_t s;
            std::cin >> s;
            unsigned good = 0, bad = 0;
            for (uint32_t x = 0; x < 256; ++x)
                for (uint32_t y = 0; y < 256; ++y) {
                    good += aesw::mult_hit(2, x, y, x ^ y, tab) && aesw::mult_bin(2, x, y) == 512 + 256 * x + y;
                    bad += aesw::mult_hit(2, x, y, x ^ y ^ (1 + (x * 31 + y + s) % 255), tab);
                }
            std::printf("%u %u\n", good, bad);
        } else if (cmd == "s") {
            using namespace aesw;
            unsigned once = 0, over = 0, clash = 0, covered = 0, stray = 0, back = 0;
            std::vector<uint32_t> bin_at[2] = {std::vector<uint32_t>(MULT_COUNTERS, MULT_NO_BIN), std::vector<uint32_t>(MULT_COUNTERS, MULT_NO_BIN)};
            for (uint32_t t = 1; t <= 5; ++t)
                for (uint32_t x = 0; x < 256; ++x)
                    for (uint32_t y = 0; y < 256; ++y) {
                        once += mult_half_owns(0, t, x) != mult_half_owns(1, t, x);
                        const uint32_t h = mult_half_owns(0, t, x) ? 0 : 1, at = mult_counter(h, t, x, y), bin = mult_bin(t, x, y);
                        if (at >= MULT_COUNTERS) { ++over; continue; }
                        clash += bin_at[h][at] != MULT_NO_BIN && bin_at[h][at] != bin;
                        bin_at[h][at] = bin;
                    }
            std::vector<unsigned> times(MULT_BINS, 0);
            for (uint32_t h = 0; h < 2; ++h)
                for (uint32_t i = 0; i < mult_flush_ranges(h); ++i) {
                    const MultFlushRange r = mult_flush_range(h, i);
                    for (uint32_t j = 0; j < r.length; ++j) {
                        if (r.bin + j >= MULT_ZERO_ROW || r.counter + j >= MULT_COUNTERS) { ++stray; continue; }
                        ++times[r.bin + j];
                        back += bin_at[h][r.counter + j] != r.bin + j;
                    }
                }
            for (uint32_t b = 0; b < MULT_ZERO_ROW; ++b) covered += times[b] == 1;
            std::printf("%u %u %u %u %u %u\n", once, over, clash, covered, stray + times[MULT_ZERO_ROW], back);
        }
    }
    return 0;
}
