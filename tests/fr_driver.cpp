// Driver of tests/test_fr_header.py: csrc/aesw_fr.h alone (no ROCm include, no other header of the project).
//   fr_driver IN OUT   IN: n records of two cells (64 bytes); OUT: per record fr_mul | fr_add (64 bytes) and, after all records,
//                      n bytes: bit 0 / bit 1 = fr_is_canonical of the first / the second cell.
// fr_mul and fr_add are only called on canonical pairs; the other records get zero cells.
//   fr_driver --byte-table OUT   OUT: the 256 cells of fr_byte_table(), 8 192 bytes
#include <cstdio>
#include <cstring>
#include <vector>

#include "aesw_fr.h"

int main(int argc, char **argv) {
    using namespace aesw;
    if (argc != 3) return 2;
    if (!std::strcmp(argv[1], "--byte-table")) {
        const FrByteTable t = fr_byte_table();
        FILE *o = std::fopen(argv[2], "wb");
        if (!o || std::fwrite(t.cell, 1, sizeof t.cell, o) != sizeof t.cell) return 2;
        std::fclose(o);
        return 0;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> in;
    unsigned char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    if (in.size() % 64) return 2;
    const size_t n = in.size() / 64;
    std::vector<unsigned char> out(n * 64 + n, 0);
    for (size_t i = 0; i < n; ++i) {
        Fr a, b;
        std::memcpy(&a, &in[i * 64], 32);
        std::memcpy(&b, &in[i * 64 + 32], 32);
        const bool ca = fr_is_canonical(a), cb = fr_is_canonical(b);
        out[n * 64 + i] = (unsigned char)(ca | cb << 1);
        if (!ca || !cb) continue;
        const Fr m = fr_mul(a, b), s = fr_add(a, b);
        std::memcpy(&out[i * 64], &m, 32);
        std::memcpy(&out[i * 64 + 32], &s, 32);
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
