// Compiled by tests/test_vacc_model.py with g++ and nothing but csrc/ on the include path: csrc/aesw_vacc.h is pure host code.
// Prints, per entry of the VALUES check table, the words of aesw_vals_check.h's image, the words build_vacc_table rebased onto
// the counting image, and the slab row both name.
#include <cstdio>

#include "aesw_vacc.h"

int main() {
    using namespace aesw;
    static uint32_t orig[2 * VALS_ROWS], t[VACC_WORDS];
    static uint16_t rows[VALS_ROWS];
    if (build_values_check_table(orig, rows) != VALS_ROWS || build_vacc_table(t) != 0) return 1;
    std::printf("%d %d %d %d %d %d %d\n", VALS_ROWS, VALS_BI, VACC_KEY_DROP, VACC_O_KZ, VACC_O_W, VACC_BI, VACC_IMG);
    for (int e = 0; e < VALS_ROWS; ++e)
        std::printf("%u %u %u %u %u %u\n", orig[2 * e], orig[2 * e + 1], t[2 * e], t[2 * e + 1], (unsigned)rows[e], vacc_slab_row(t, (uint32_t)e));
    return 0;
}
