// vanish_driver.cpp -- csrc/aesw_vanish.h alone under g++ (tests/test_vanish_model.py): the rules as text, and the quotient executed
// on the CPU segment by segment through the header's own functions -- what the kernels of libaesw_vanish.so do, row by row.  A
// program of its own, so that it can be built under -fsanitize=address,undefined.
//   segments N_SETS CHUNK_LEN                      per segment: kind set len products overhead; then: their sums and quot_products_per_row
//   sizes N_SETS CHUNK_LEN                         the bytes of the scalars block
//   offset TABLE INDEX                             the byte offset of an entry of the block, or -1
//   scalars N_SETS CHUNK_LEN IN OUT                IN: theta, beta, gamma, y; OUT: the block
//   run K EXT_K ZETA_SEL N_SETS CHUNK_LEN N_ROWS IN OUT   IN: every column group in quot_numerator's order, then theta, beta, gamma, y, then
//                                                  one column more, an arbitrary acc_in.  On every row: the segments in their order are
//                                                  quot_numerator (else exit 6), and each segment from acc_in is acc_in * y^len + the
//                                                  segment from 0 (else exit 7).  OUT: the quotient after the division.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "aesw_vanish.h"

using namespace aesw;

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const auto arg = [&](int i) { return i < argc ? (uint32_t)std::strtol(argv[i], nullptr, 10) : 0u; };
    if (mode == "segments") {
        for (uint32_t i = 0; i < vanish_segments(arg(2), arg(3)); ++i) {
            const VanishSegment seg = vanish_segment(arg(2), arg(3), i);
            std::printf("%u %u %u %u %d\n", seg.kind, seg.set, vanish_segment_len(seg.kind, arg(2), arg(3)), vanish_segment_products(seg, arg(2), arg(3)), vanish_segment_overhead(seg));
        }
        std::printf("%u %u %d\n", vanish_products_per_row(arg(2), arg(3)), quot_products_per_row(arg(2), arg(3)), vanish_overhead_per_row(arg(2), arg(3)));
    } else if (mode == "sizes") {
        std::printf("%llu\n", (unsigned long long)vanish_scalars_bytes(arg(2), arg(3)));
    } else if (mode == "offset") {
        const uint64_t at = vanish_table_at(arg(2), arg(3));
        std::printf("%lld\n", at == ~(uint64_t)0 ? -1ll : (long long)(at * sizeof(Fr)));
    } else if (mode == "scalars" && argc == 6) {
        if (!vanish_scalars_bytes(arg(2), arg(3))) return 4;
        std::vector<Fr> in(4), out(vanish_scalars_cells(arg(2), arg(3)));
        FILE *f = std::fopen(argv[4], "rb");
        if (!f || std::fread(in.data(), sizeof(Fr), in.size(), f) != in.size()) return 3;
        std::fclose(f);
        for (uint32_t at = 0; at < out.size(); ++at) out[at] = vanish_scalar_cell(at, arg(2), arg(3), in[0], in[1], in[2], in[3]);
        f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(out.data(), sizeof(Fr), out.size(), f) != out.size()) return 3;
        std::fclose(f);
    } else if (mode == "run" && argc == 10) {
        const QuotShape q{arg(2), arg(3), arg(4), arg(5), arg(6), arg(7)};
        if (!quot_shape_ok(q)) return 4;
        const size_t rows = (size_t)1 << q.ext_k;
        size_t first[QUOT_GROUPS + 1] = {0};
        for (uint32_t g = 0; g < QUOT_GROUPS; ++g) first[g + 1] = first[g] + quot_group_columns(g, q.n_sets, q.chunk_len) * rows;
        std::vector<Fr> in(first[QUOT_GROUPS] + 4 + rows), out(rows), tables(quot_tables(q.k, q.ext_k).cells), block(vanish_scalars_cells(q.n_sets, q.chunk_len));
        FILE *f = std::fopen(argv[8], "rb");
        if (!f || std::fread(in.data(), sizeof(Fr), in.size(), f) != in.size()) return 3;
        std::fclose(f);
        for (uint32_t i = 0; i < tables.size(); ++i) tables[i] = quot_table_cell(q.k, q.ext_k, q.zeta_sel, i);
        const Fr theta = in.at(first[QUOT_GROUPS]), beta = in.at(first[QUOT_GROUPS] + 1), gamma = in.at(first[QUOT_GROUPS] + 2), y = in.at(first[QUOT_GROUPS] + 3);
        for (uint32_t at = 0; at < block.size(); ++at) block[at] = vanish_scalar_cell(at, q.n_sets, q.chunk_len, theta, beta, gamma, y);
        const Fr *seeded = &in.at(first[QUOT_GROUPS] + 4);
        const auto table = [&](uint32_t at) { return tables.at(at); };
        const auto scalar = [&](uint32_t at) { return block.at(at); };
        const auto plain = [&](uint32_t group, uint32_t column, uint32_t row) {
            if (group >= QUOT_GROUPS || column >= quot_group_columns(group, q.n_sets, q.chunk_len) || row >= rows) std::exit(5);
            return in.at(first[group] + column * rows + row);
        };
        const auto load = [&](uint32_t group, uint32_t column, uint32_t row) {  // with the permutation's values resolved
            if (group != VANISH_VALUES) return plain(group, column, row);
            if (column >= sigma_columns(q.n_sets)) std::exit(5);
            return plain(vanish_values_group(q.n_sets, column), vanish_values_column(q.n_sets, column), row);
        };
        const auto segment = [&](const VanishSegment &seg, uint32_t j, const Fr &acc, const Fr &x) {
            return seg.kind == VANISH_HEAD ? vanish_head(q, j, load, scalar) : seg.kind == VANISH_PERM ? vanish_perm(q, seg.set, j, acc, x, load, scalar)
                 : seg.kind == VANISH_LOOKUP ? vanish_lookup(q, seg.set, j, acc, load, scalar) : vanish_divide(q.k, q.ext_k, j, acc, table);
        };
        const uint32_t n = vanish_segments(q.n_sets, q.chunk_len);
        for (uint32_t j = 0; j < rows; ++j) {
            const Fr x = quot_point(q.k, q.ext_k, j, table);
            Fr acc = FR_ZERO;
            for (uint32_t i = 0; i + 1 < n; ++i) {
                const VanishSegment seg = vanish_segment(q.n_sets, q.chunk_len, i);
                if (i) {  // from an arbitrary acc_in: acc_in * y^len + the segment from 0
                    const Fr power = scalar(VANISH_AT_Y_POW + seg.kind);
                    if (!fr_eq(segment(seg, j, seeded[j], x), fr_add(fr_mul(seeded[j], power), segment(seg, j, FR_ZERO, x)))) return 7;
                }
                acc = segment(seg, j, acc, x);
            }
            if (!fr_eq(acc, quot_numerator(q, j, x, theta, beta, gamma, y, plain))) return 6;
            out[j] = segment(vanish_segment(q.n_sets, q.chunk_len, n - 1), j, acc, x);
        }
        f = std::fopen(argv[9], "wb");
        if (!f || std::fwrite(out.data(), sizeof(Fr), out.size(), f) != out.size()) return 3;
        std::fclose(f);
    } else {
        return 2;
    }
    return 0;
}
