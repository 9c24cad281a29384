// The rules header of libaesw_sigma.so (csrc/aesw_sigma.h) on the CPU: g++ alone, no ROCm include, no GPU.  tests/test_sigma_model.py
// holds what this prints against tests/sigma_model.py.
//   constants          prints g, the 2^28-th root, delta as plain residues in hex (Montgomery form taken off by a product with 1)
//   omega <k>          omega_k
//   cell <k> <at>...   the table cell `at` of sigma_table_cell
//   split <k> <i>...   low index, high index, and omega^i as the product of the two table cells
//   index <k> <n_cols> <m>...   col, row, in range
//   geometry <k> <n_cols> <chunk_len> <n_rows>   sets, last row, chunks, stride, tables bytes, workspace bytes, then first/end of every set
//   order <n_sets>     columns, then source of every column, then column of every advice column
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "aesw_sigma.h"

using namespace aesw;

static void print(const Fr &mont) {
    Fr one = FR_ZERO;
    one.l[0] = 1;
    const Fr v = fr_mul(mont, one);  // v * 2^256 * 1 / 2^256
    for (int i = FR_LIMBS - 1; i >= 0; --i) std::printf("%08x", v.l[i]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const auto arg = [&](int i) { return (uint32_t)std::strtoull(argv[i], nullptr, 0); };
    if (!std::strcmp(argv[1], "constants")) {
        print(SIGMA_GENERATOR);
        print(SIGMA_ROOT);
        print(SIGMA_DELTA);
    } else if (!std::strcmp(argv[1], "omega")) {
        print(sigma_omega(arg(2)));
    } else if (!std::strcmp(argv[1], "cell")) {
        for (int i = 3; i < argc; ++i) print(sigma_table_cell(arg(2), arg(i)));
    } else if (!std::strcmp(argv[1], "split")) {
        const uint32_t k = arg(2);
        for (int i = 3; i < argc; ++i) {
            const uint32_t lo = sigma_low_index(arg(i)), hi = sigma_high_index(arg(i));
            std::printf("%u %u ", lo, hi);
            print(fr_mul(sigma_table_cell(k, lo), sigma_table_cell(k, sigma_low_cells(k) + hi)));
        }
    } else if (!std::strcmp(argv[1], "index")) {
        const uint32_t k = arg(2), n_cols = arg(3);
        for (int i = 4; i < argc; ++i)
            std::printf("%u %u %d %u\n", sigma_cell_col(k, arg(i)), sigma_cell_row(k, arg(i)), (int)sigma_cell_in_range(k, n_cols, arg(i)),
                        sigma_cell_index(k, sigma_cell_col(k, arg(i)), sigma_cell_row(k, arg(i))));
    } else if (!std::strcmp(argv[1], "geometry")) {
        const uint32_t k = arg(2), n_cols = arg(3), chunk_len = arg(4), n_rows = arg(5);
        const bool ok = sigma_shape_ok(k, n_cols) && sigma_chunk_len_ok(chunk_len);
        std::printf("%u %u %u %u %llu %llu\n", ok ? sigma_sets(n_cols, chunk_len) : 0u, ok ? sigma_last_row(k, n_rows) : 0u, ok ? sigma_chunks(k, n_rows) : 0u,
                    ok ? sigma_chunk_stride(k) : 0u, (unsigned long long)sigma_tables_bytes(k, n_cols), (unsigned long long)sigma_workspace_bytes(k, n_cols, chunk_len));
        if (ok)
            for (uint32_t s = 0; s < sigma_sets(n_cols, chunk_len); ++s) std::printf("%u %u\n", sigma_set_first(s, chunk_len), sigma_set_end(s, chunk_len, n_cols));
    } else if (!std::strcmp(argv[1], "order")) {
        const uint32_t n_sets = arg(2);
        std::printf("%u\n", sigma_columns(n_sets));
        for (uint32_t c = 0; c < sigma_columns(n_sets); ++c) std::printf("%u ", sigma_source_of_column(n_sets, c));
        std::printf("\n");
        for (uint32_t a = 0; a <= 3 * n_sets; ++a) std::printf("%u ", sigma_column_of_advice(n_sets, a));
        std::printf("\n");
    } else {
        return 2;
    }
    return 0;
}
