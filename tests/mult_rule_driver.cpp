// tests/test_mult_rule.py: csrc/aesw_mult.h compiled alone (no ROCm include), answering on stdin / stdout.
//   first line:  768 table bytes (sbox | mul2 | mul3) as decimals
//   "r t x y z": one (tag, x, y, z)                       -> "bin hit"
//   "m t":       every (x, y) of a one-operand tag 3..5   -> the number of hits, and of hits whose bin is not first + x
//   "x s":       the Xor tag, every (x, y) with z = x ^ y and with z = x ^ y ^ (1 + (x * 31 + y + s) % 255)
//                -> hits of the first kind whose bin is 512 + 256 x + y, hits of the second kind
#include <cstdio>
#include <iostream>
#include <string>

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
        }
    }
    return 0;
}
