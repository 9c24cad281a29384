// tests/fr_inv_driver.cpp -- csrc/aesw_fr.h's inverse and comparisons alone, for tests/test_fr_inverse.py: no ROCm, no GPU.
// usage: fr_inv_driver IN OUT -- IN holds n cells of 32 bytes; OUT gets per cell fr_inv(a) and fr_mul(fr_inv(a), a), 64 bytes,
// then n flag bytes: bit 0 fr_is_zero(a), bit 1 fr_eq(a, a), bit 2 fr_eq(a, FR_ONE), bit 3 fr_eq(a, fr_inv(a)).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "aesw_fr.h"

using namespace aesw;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<Fr> a;
    Fr cell;
    while (fread(&cell, sizeof cell, 1, in) == 1) a.push_back(cell);
    fclose(in);
    std::vector<Fr> out;
    std::vector<unsigned char> flags;
    for (const Fr &v : a) {
        const Fr i = fr_inv(v);
        out.push_back(i);
        out.push_back(fr_mul(i, v));
        flags.push_back((unsigned char)((fr_is_zero(v) ? 1 : 0) | (fr_eq(v, v) ? 2 : 0) | (fr_eq(v, FR_ONE) ? 4 : 0) | (fr_eq(v, i) ? 8 : 0)));
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 3;
    if (!out.empty() && fwrite(out.data(), sizeof(Fr), out.size(), o) != out.size()) return 4;
    if (!flags.empty() && fwrite(flags.data(), 1, flags.size(), o) != flags.size()) return 4;
    fclose(o);
    return 0;
}
