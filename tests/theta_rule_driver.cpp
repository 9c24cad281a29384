// Driver of tests/test_theta_model.py: csrc/aesw_theta.h alone (no ROCm include).
//   theta_rule_driver table TAB768 FR_LUT THETA OUT              OUT: [3][66561][32] bytes, then 5 bytes theta_table_of_tag(1 ... 5)
//   theta_rule_driver rows TAB768 OUT                            OUT: [4][66561] bytes: tag, a, b, c of theta_table_row
//   theta_rule_driver index U PAD OUT                            OUT: U words theta_table_index(i, PAD)
//   theta_rule_driver inputs K N_SETS N_BLOCKS PACKED TAB768 X Y Z KX KY KZ OUT   (KX == "-": no key slab)
//                                                                OUT: [N_SETS][5][2^K] words; stdout: lookups misses first_miss
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_theta.h"

using namespace aesw;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    if (std::string(path) == "-") return v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}
static void dump(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) std::exit(2);
    std::fclose(f);
}
static Fr cell(const std::vector<uint8_t> &lut, uint32_t v) {
    Fr c;
    std::memcpy(&c, &lut[32 * v], 32);
    return c;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table" && argc == 6) {
        const auto tab = slurp(argv[2]), lut = slurp(argv[3]), th = slurp(argv[4]);
        if (tab.size() != 768 || lut.size() != 256 * 32 || th.size() != 32) return 2;
        const Fr theta = cell(th, 0);
        std::vector<uint8_t> out((size_t)THETA_TABLES * MULT_BINS * 32 + THETA_TAGS, 0);
        if (fr_is_canonical(theta))
            for (uint32_t j = 0; j < THETA_TABLES; ++j)
                for (uint32_t r = 0; r < MULT_BINS; ++r) {
                    const ThetaTableRow row = theta_table_row(r, tab.data());
                    const Fr c = theta_compress(theta, cell(lut, row.tag), cell(lut, row.a), cell(lut, row.b), cell(lut, row.c), theta_arity(j));
                    std::memcpy(&out[((size_t)j * MULT_BINS + r) * 32], &c, 32);
                }
        for (uint32_t t = 1; t <= THETA_TAGS; ++t) out[(size_t)THETA_TABLES * MULT_BINS * 32 + t - 1] = (uint8_t)theta_table_of_tag(t);
        dump(argv[5], out.data(), out.size());
        return 0;
    }
    if (mode == "rows" && argc == 4) {
        const auto tab = slurp(argv[2]);
        if (tab.size() != 768) return 2;
        std::vector<uint8_t> out((size_t)4 * MULT_BINS);
        for (uint32_t r = 0; r < MULT_BINS; ++r) {
            const ThetaTableRow row = theta_table_row(r, tab.data());
            out[r] = (uint8_t)row.tag; out[MULT_BINS + r] = (uint8_t)row.a; out[2 * (size_t)MULT_BINS + r] = (uint8_t)row.b; out[3 * (size_t)MULT_BINS + r] = (uint8_t)row.c;
        }
        dump(argv[3], out.data(), out.size());
        return 0;
    }
    if (mode == "index" && argc == 5) {
        const uint32_t u = (uint32_t)std::atol(argv[2]), pad = (uint32_t)std::atol(argv[3]);
        std::vector<uint32_t> out(u);
        for (uint32_t i = 0; i < u; ++i) out[i] = theta_table_index(i, pad);
        dump(argv[4], out.data(), out.size() * 4);
        return 0;
    }
    if (mode == "inputs" && argc == 14) {
        const uint32_t k = (uint32_t)std::atol(argv[2]), n_sets = (uint32_t)std::atol(argv[3]);
        const uint64_t n_blocks = (uint64_t)std::atoll(argv[4]);
        const int packed = std::atoi(argv[5]);
        const auto tab = slurp(argv[6]), x = slurp(argv[7]), y = slurp(argv[8]), z = slurp(argv[9]), kx = slurp(argv[10]), ky = slurp(argv[11]),
                   kz = slurp(argv[12]);
        const Placement place(k);
        if (n_blocks > place.total(n_sets)) return 3;
        const SlabStrides st = slab_strides(packed ? PACKED : DENSE);
        const bool with_keys = !kx.empty() && mult_has_key_rows(k);
        const uint8_t *pkx = with_keys ? kx.data() : nullptr, *pky = with_keys ? ky.data() : nullptr, *pkz = with_keys ? kz.data() : nullptr;
        const uint64_t rows = (uint64_t)1 << k;
        std::vector<uint32_t> out((size_t)n_sets * THETA_TAGS * rows);
        uint64_t lookups = 0, misses = 0, first = ~0ull;
        for (uint32_t s = 0; s < n_sets; ++s) {
            ColumnSource cs[3];
            for (uint32_t c = 0; c < 3; ++c) cs[c] = column_source(place, 3 * s + c, n_sets, pkx, pky, pkz, x.data(), y.data(), z.data(), st.x, st.y, st.z);
            for (uint64_t i = 0; i < rows; ++i) {
                const ThetaInput in = theta_input_row(cs, packed, with_keys, (uint32_t)i, n_blocks, tab.data());
                for (uint32_t t = 1; t <= THETA_TAGS; ++t) out[(((size_t)s * THETA_TAGS + t - 1) << k) + i] = in.tag == t ? in.cell : MULT_ZERO_ROW;
                lookups += in.tag != 0;
                misses += in.cell == THETA_MISS;
                first = in.miss_key < first ? in.miss_key : first;
            }
        }
        dump(argv[13], out.data(), out.size() * 4);
        std::printf("%llu %llu %llu\n", (unsigned long long)lookups, (unsigned long long)misses, (unsigned long long)first);
        return 0;
    }
    return 2;
}
