// field_driver.cpp -- csrc/aesw_fr.h and csrc/aesw_fq.h over csrc/aesw_mont.h behind a program of its own
// (tests/test_field_headers.py): no ROCm include, no other header of the project.
//   field_driver fr|fq IN OUT       IN: pairs of 32-byte values (a, b); OUT: per pair mont_mul | mont_add | mont_sub (96 bytes), all
//                                   zero unless both are canonical, and behind them all one flag byte a pair: bit 0 a is
//                                   canonical, bit 1 b is.
//   field_driver fr|fq --inv IN OUT IN: 32-byte values a; OUT: per value the field's inverse (32 bytes), zero unless a is canonical.
//   field_driver fr|fq --one OUT    OUT: the Montgomery form of 1 and the plain 1 of the field's trait, 64 bytes
//   field_driver --byte-table OUT   OUT: the 256 cells of fr_byte_table(), 8 192 bytes
#include <cstdio>
#include <cstring>
#include <vector>

#include "aesw_fq.h"
#include "aesw_fr.h"

using namespace aesw;

static Fr inverse(const Fr &a) { return fr_inv(a); }
static Fq inverse(const Fq &a) { return fq_inv(a); }

template <class F>
static bool read_all(const char *path, std::vector<F> &in) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    F v;
    while (std::fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
    std::fclose(f);
    return true;
}

template <class F>
static bool write_all(const char *path, const std::vector<F> &out, const std::vector<unsigned char> &flags) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = (out.empty() || std::fwrite(out.data(), sizeof(F), out.size(), f) == out.size()) &&
                    (flags.empty() || std::fwrite(flags.data(), 1, flags.size(), f) == flags.size());  // an empty vector's data() may be null
    return std::fclose(f) == 0 && ok;
}

template <class F>
static int run(int argc, char **argv) {  // argv: what follows the field's name
    const F zero = MontField<F>::ZERO;
    std::vector<F> in, out;
    std::vector<unsigned char> flags;
    if (argc == 2 && !std::strcmp(argv[0], "--one")) {
        out = {MontField<F>::ONE, MontField<F>::RAW_ONE};
        return write_all(argv[1], out, flags) ? 0 : 2;
    }
    if (argc == 3 && !std::strcmp(argv[0], "--inv")) {
        if (!read_all(argv[1], in)) return 2;
        for (const F &a : in) out.push_back(mont_is_canonical(a) ? inverse(a) : zero);
        return write_all(argv[2], out, flags) ? 0 : 2;
    }
    if (argc != 2 || !read_all(argv[0], in) || in.size() % 2) return 2;
    for (size_t i = 0; i < in.size(); i += 2) {
        const F &a = in[i], &b = in[i + 1];
        const bool ca = mont_is_canonical(a), cb = mont_is_canonical(b);
        flags.push_back((unsigned char)(ca | cb << 1));
        const bool both = ca && cb;  // the arithmetic is defined on canonical values
        out.push_back(both ? mont_mul(a, b) : zero);
        out.push_back(both ? mont_add(a, b) : zero);
        out.push_back(both ? mont_sub(a, b) : zero);
    }
    return write_all(argv[1], out, flags) ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--byte-table")) {
        const FrByteTable t = fr_byte_table();
        return write_all(argv[2], std::vector<Fr>(t.cell, t.cell + 256), {}) ? 0 : 2;
    }
    if (argc < 4) return 2;
    if (!std::strcmp(argv[1], "fr")) return run<Fr>(argc - 2, argv + 2);
    if (!std::strcmp(argv[1], "fq")) return run<Fq>(argc - 2, argv + 2);
    return 2;
}
