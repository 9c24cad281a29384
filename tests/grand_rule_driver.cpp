// tests/grand_rule_driver.cpp -- csrc/aesw_grand.h alone, for tests/test_grand_model.py: no ROCm include, no GPU.
//   grand_rule_driver rows IN OUT        IN: n x (t_in, t_tab, inv_a, inv_s, beta, gamma) cells; OUT: n cells grand_row(...)
//   grand_rule_driver batch B IN OUT     IN: the cell c, then n cells x; OUT: inv(x + c) by grand_batch_invert<B> over consecutive
//                                        batches (the last one filled with zero sums); prints the zero sums among the n
//   grand_rule_driver geometry K N_ROWS N_SETS    prints last_row chunks stride workspace_bytes rows_per_lane batch
//   grand_rule_driver index X...         prints grand_row_of_index(x) and grand_argument_key(x) of every x
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "aesw_grand.h"

using namespace aesw;

static std::vector<Fr> read_cells(const char *path) {
    std::vector<Fr> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(3);
    Fr c;
    while (fread(&c, sizeof c, 1, f) == 1) v.push_back(c);
    fclose(f);
    return v;
}

static void write_cells(const char *path, const std::vector<Fr> &v) {
    FILE *f = fopen(path, "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(Fr), v.size(), f) != v.size())) exit(4);
    fclose(f);
}

template <int B>
static uint32_t invert_all(const std::vector<Fr> &x, const Fr &c, std::vector<Fr> &out) {
    uint32_t zeros = 0;
    const size_t n = x.size();
    for (size_t r0 = 0; r0 < n; r0 += B) {
        uint32_t in_range_zeros = 0;
        grand_batch_invert<B>([&](int i) { return r0 + i < n ? fr_add(x[r0 + i], c) : FR_ZERO; },
                              [&](int i, const Fr &v) {
                                  if (r0 + i < n) {
                                      out[r0 + i] = v;
                                      in_range_zeros += fr_is_zero(v) ? 1u : 0u;
                                  }
                              });
        zeros += in_range_zeros;
    }
    return zeros;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "rows") && argc == 4) {
        const std::vector<Fr> in = read_cells(argv[2]);
        std::vector<Fr> out;
        for (size_t i = 0; i + 6 <= in.size(); i += 6) out.push_back(grand_row(in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4], in[i + 5]));
        write_cells(argv[3], out);
        return 0;
    }
    if (!strcmp(argv[1], "batch") && argc == 5) {
        std::vector<Fr> x = read_cells(argv[3]);
        if (x.empty()) return 2;
        const Fr c = x[0];
        x.erase(x.begin());
        std::vector<Fr> out(x.size(), FR_ONE);
        uint32_t zeros = 0;
        switch (atoi(argv[2])) {
        case 1: zeros = invert_all<1>(x, c, out); break;
        case 3: zeros = invert_all<3>(x, c, out); break;
        case 8: zeros = invert_all<8>(x, c, out); break;
        case 16: zeros = invert_all<16>(x, c, out); break;
        default: return 2;
        }
        write_cells(argv[4], out);
        printf("%u\n", zeros);
        return 0;
    }
    if (!strcmp(argv[1], "geometry") && argc == 5) {
        const uint32_t k = (uint32_t)atoi(argv[2]), n_rows = (uint32_t)strtoul(argv[3], nullptr, 10), n_sets = (uint32_t)atoi(argv[4]);
        const bool ok = grand_k_ok(k);
        printf("%u %u %u %llu %u %u\n", ok ? grand_last_row(k, n_rows) : 0u, ok ? grand_chunks(k, n_rows) : 0u, ok ? grand_chunk_stride(k) : 0u,
               (unsigned long long)grand_workspace_bytes(k, n_sets), GRAND_ROWS_PER_LANE, GRAND_BATCH);
        return 0;
    }
    if (!strcmp(argv[1], "index")) {
        for (int i = 2; i < argc; ++i) {
            const uint32_t x = (uint32_t)strtoul(argv[i], nullptr, 10);
            printf("%u %llu\n", grand_row_of_index(x), (unsigned long long)grand_argument_key(x));
        }
        return 0;
    }
    return 2;
}
