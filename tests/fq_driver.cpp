// fq_driver.cpp -- csrc/aesw_fq.h alone behind a program of its own (tests/test_fq_header.py): in.bin holds pairs of 32-byte
// values (a, b); out.bin gets, per pair, fq_mul, fq_add, fq_sub and fq_inv(a) -- 128 bytes -- and behind them all one flag byte a
// pair: bit 0 a is canonical, bit 1 b is.
#include <cstdio>
#include <cstring>
#include <vector>

#include "aesw_fq.h"

using namespace aesw;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<Fq> in;
    Fq v;
    while (fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
    fclose(f);
    const size_t n = in.size() / 2;
    std::vector<Fq> out;
    std::vector<unsigned char> flags;
    for (size_t i = 0; i < n; ++i) {
        const Fq &a = in[2 * i], &b = in[2 * i + 1];
        const bool ca = fq_is_canonical(a), cb = fq_is_canonical(b);
        flags.push_back((unsigned char)(ca | cb << 1));
        const bool both = ca && cb;  // the arithmetic is defined on canonical values
        out.push_back(both ? fq_mul(a, b) : FQ_ZERO);
        out.push_back(both ? fq_add(a, b) : FQ_ZERO);
        out.push_back(both ? fq_sub(a, b) : FQ_ZERO);
        out.push_back(ca ? fq_inv(a) : FQ_ZERO);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), sizeof(Fq), out.size(), f) == out.size() && fwrite(flags.data(), 1, flags.size(), f) == flags.size();
    fclose(f);
    return ok ? 0 : 2;
}
