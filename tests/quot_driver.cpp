// quot_driver.cpp -- csrc/aesw_quot.h alone under g++ (tests/test_quot_model.py): the rules as text, and the quotient executed on
// the CPU through the header's own functions -- quot_table_cell, quot_point, quot_numerator, quot_vanish_index: what a kernel
// of the quotient does, row by row.  A program of its own, so that it can be built under -fsanitize=address,undefined.
//   rot K EXT_K J R | vanish K EXT_K J | products N_SETS CHUNK_LEN | columns N_SETS CHUNK_LEN | ok K EXT_K ZETA_SEL N_SETS CHUNK_LEN N_ROWS
//   sizes K EXT_K                                   the bytes of the tables and where the three of them start
//   table K EXT_K ZETA_SEL AT...                    cells of the tables
//   label K N_COLS C I ENTRY                        the image of a mapping entry and its label, from the permutation's tables
//   run K EXT_K ZETA_SEL N_SETS CHUNK_LEN N_ROWS IN OUT   IN: every column group in the call's order, then theta, beta, gamma, y
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "aesw_quot.h"

using namespace aesw;

static void print_cell(const Fr &v) {  // the 256-bit number the limbs spell, Montgomery form as it lies
    for (int i = FR_LIMBS - 1; i >= 0; --i) std::printf("%08x", v.l[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const auto arg = [&](int i) { return i < argc ? (uint32_t)std::strtol(argv[i], nullptr, 10) : 0u; };
    if (mode == "rot") {
        std::printf("%u\n", quot_rot(arg(2), arg(3), arg(4), (int32_t)arg(5)));
    } else if (mode == "vanish") {
        std::printf("%u\n", quot_vanish_index(arg(2), arg(3), arg(4)));
    } else if (mode == "products") {
        std::printf("%u\n", quot_products_per_row(arg(2), arg(3)));
    } else if (mode == "columns") {
        for (uint32_t g = 0; g < QUOT_GROUPS; ++g) std::printf("%u ", quot_group_columns(g, arg(2), arg(3)));
        std::printf("%u\n", quot_columns(arg(2), arg(3)));
    } else if (mode == "ok") {
        std::printf("%d\n", (int)quot_shape_ok(QuotShape{arg(2), arg(3), arg(4), arg(5), arg(6), arg(7)}));
    } else if (mode == "sizes") {
        const QuotTables t = quot_tables(arg(2), arg(3));
        std::printf("%llu %u %u %u %u\n", (unsigned long long)quot_tables_bytes(arg(2), arg(3)), t.vanish_at, t.low_at, t.high_at, t.cells);
    } else if (mode == "table") {
        for (int i = 5; i < argc; ++i) print_cell(quot_table_cell(arg(2), arg(3), arg(4), arg(i)));
    } else if (mode == "label" && argc == 7) {
        const uint32_t k = arg(2), n_cols = arg(3), image = quot_sigma_image(k, n_cols, arg(4), arg(5), arg(6));
        std::printf("%u\n", image);
        print_cell(quot_sigma_label(k, image, [&](uint32_t at) { return sigma_table_cell(k, at); }));
    } else if (mode == "run" && argc == 10) {
        const QuotShape q{arg(2), arg(3), arg(4), arg(5), arg(6), arg(7)};
        if (!quot_shape_ok(q)) return 4;
        const size_t rows = (size_t)1 << q.ext_k;
        size_t first[QUOT_GROUPS + 1] = {0};
        for (uint32_t g = 0; g < QUOT_GROUPS; ++g) first[g + 1] = first[g] + quot_group_columns(g, q.n_sets, q.chunk_len) * rows;
        std::vector<Fr> in(first[QUOT_GROUPS] + 4), out(rows), tables(quot_tables(q.k, q.ext_k).cells);
        FILE *f = std::fopen(argv[8], "rb");
        if (!f || std::fread(in.data(), sizeof(Fr), in.size(), f) != in.size()) return 3;
        std::fclose(f);
        for (uint32_t i = 0; i < tables.size(); ++i) tables[i] = quot_table_cell(q.k, q.ext_k, q.zeta_sel, i);
        const Fr theta = in.at(first[QUOT_GROUPS]), beta = in.at(first[QUOT_GROUPS] + 1), gamma = in.at(first[QUOT_GROUPS] + 2), y = in.at(first[QUOT_GROUPS] + 3);
        const auto table = [&](uint32_t at) { return tables.at(at); };
        const auto load = [&](uint32_t group, uint32_t column, uint32_t row) {
            if (column >= quot_group_columns(group, q.n_sets, q.chunk_len) || row >= rows) std::exit(5);
            return in.at(first[group] + column * rows + row);
        };
        for (uint32_t j = 0; j < rows; ++j)
            out[j] = fr_mul(quot_numerator(q, j, quot_point(q.k, q.ext_k, j, table), theta, beta, gamma, y, load),
                            table(quot_tables(q.k, q.ext_k).vanish_at + quot_vanish_index(q.k, q.ext_k, j)));
        f = std::fopen(argv[9], "wb");
        if (!f || std::fwrite(out.data(), sizeof(Fr), out.size(), f) != out.size()) return 3;
        std::fclose(f);
    } else {
        return 2;
    }
    return 0;
}
