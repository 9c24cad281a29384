// ntt_driver.cpp -- csrc/aesw_ntt.h alone under g++ (tests/test_ntt_model.py): the constants, the plan and the sizes as text, and
// the transforms executed on the CPU through the header's own index and twiddle functions -- what ntt/aesw_ntt.hip's pass kernel
// does, workgroup by workgroup and slot by slot, with fr_mul, fr_add and fr_sub of aesw_fr.h.  A program of its own, so that it
// can be built under -fsanitize=address,undefined.
//   constants | omega K | scale K V | plan | sizes MAX_K K N_COLS
//   run NAME K EXT_K ZETA_SEL MAX_K IN OUT     NAME: l2c c2l c2e e2c; IN, OUT: files of 32-byte cells
//   sparse K MAX_K E0 C0 E1 C1 E2 C2 ROW...    coeff_to_lagrange of three coefficients (cells as 64 hex digits), the rows asked for
//   sparse_ext K EXT_K ZETA_SEL MAX_K E0 C0 E1 C1 E2 C2 ROW...   coeff_to_extended of the same, the rows asked for, then the number of
//                                              cells extended_to_coeff of it gets wrong
//   positions K PASS W SLOT                   the column position and the load twiddle of a slot
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_ntt.h"

using namespace aesw;

static void print_cell(const Fr &v) {  // the 256-bit number the limbs spell, Montgomery form as it lies
    for (int i = FR_LIMBS - 1; i >= 0; --i) std::printf("%08x", v.l[i]);
    std::printf("\n");
}
static Fr parse_cell(const char *hex) {
    Fr v = FR_ZERO;
    if (std::strlen(hex) != 64) std::exit(2);
    for (int i = 0; i < FR_LIMBS; ++i) v.l[FR_LIMBS - 1 - i] = (uint32_t)std::strtoul(std::string(hex + 8 * i, 8).c_str(), nullptr, 16);
    return v;
}

enum : uint32_t { F_INVERSE = 1, F_ZETA_LOAD = 4, F_SCALE = 8, F_ZETA_STORE = 16 };

struct Tables {
    std::vector<Fr> cell;
    NttTables at;
    explicit Tables(uint32_t max_k) : cell(ntt_tables(max_k).cells), at(ntt_tables(max_k)) {
        for (uint32_t i = 0; i < at.cells; ++i) cell[i] = ntt_table_cell(max_k, i);
    }
    Fr root_power(uint32_t e) const { return fr_mul(cell[at.low_at + ntt_low_index(e)], cell[at.high_at + ntt_high_index(e)]); }
};

// in: 2^src_k cells, out: 2^k cells; the passes as the launcher of ntt/aesw_ntt.hip orders them
static void transform(const Tables &t, uint32_t k, uint32_t src_k, uint32_t max_k, uint32_t zeta_sel, uint32_t first, uint32_t last, const std::vector<Fr> &in,
                      std::vector<Fr> &out) {
    const bool inverse = first & F_INVERSE;
    std::vector<Fr> tile(NTT_SLOTS);
    for (uint32_t i = 0; i < ntt_passes(k); ++i) {
        const NttPass q = ntt_pass(k, i);
        const bool is_first = i == 0, is_last = i + 1 == ntt_passes(k);
        for (uint32_t w = 0; w < ntt_workgroups(k); ++w) {
            for (uint32_t slot = 0; slot < NTT_SLOTS; ++slot) {
                const uint32_t position = ntt_slot_position(q, w, slot);
                Fr v = FR_ZERO;
                if (is_first) {
                    const uint32_t src = ntt_first_source(k, position);
                    if (src >> src_k == 0) {
                        v = in.at(src);
                        const uint32_t e = first & F_ZETA_LOAD ? ntt_zeta_exponent(zeta_sel, src, false) : 0u;
                        if (e) v = fr_mul(v, t.cell[t.at.scales_at + ntt_scale_index(0, e)]);
                    }
                } else {
                    v = fr_mul(out.at(position), t.root_power(ntt_root_exponent(max_k, q.s0 + q.m, ntt_slot_twiddle(q, w, slot), inverse)));
                }
                tile.at(ntt_lds_index(slot)) = v;
            }
            for (uint32_t j = 1; j <= q.m; ++j)
                for (uint32_t b = 0; b < NTT_SLOTS / 2; ++b) {
                    const uint32_t lower = ntt_butterfly_slot(q, j, b), upper = lower + ntt_butterfly_span(q, j);
                    const Fr x = tile.at(ntt_lds_index(lower));
                    const Fr y = fr_mul(tile.at(ntt_lds_index(upper)), t.cell.at(t.at.short_at + ntt_butterfly_twiddle(q, j, lower, inverse)));
                    tile.at(ntt_lds_index(lower)) = fr_add(x, y);
                    tile.at(ntt_lds_index(upper)) = fr_sub(x, y);
                }
            for (uint32_t slot = 0; slot < NTT_SLOTS; ++slot) {
                const uint32_t position = ntt_slot_position(q, w, slot);
                Fr v = tile.at(ntt_lds_index(slot));
                if (is_last && (last & F_SCALE)) {
                    const uint32_t e = last & F_ZETA_STORE ? ntt_zeta_exponent(zeta_sel, position, true) : 0u;
                    v = fr_mul(v, t.cell.at(t.at.scales_at + ntt_scale_index(k, e)));
                }
                out.at(position) = v;
            }
        }
    }
}

static std::vector<Fr> read_cells(const char *path, size_t cells) {
    std::vector<Fr> v(cells);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(Fr), cells, f) != cells) std::exit(3);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const auto arg = [&](int i) { return i < argc ? (uint32_t)std::strtoul(argv[i], nullptr, 10) : 0u; };
    if (mode == "constants") {
        std::printf("%u\n", NTT_PASS_LOG);
        print_cell(NTT_ZETA0);
        print_cell(NTT_ZETA1);
        print_cell(NTT_INV_TWO);
    } else if (mode == "omega") {
        print_cell(sigma_omega(arg(2)));
    } else if (mode == "scale") {
        print_cell(ntt_table_cell(28, ntt_tables(28).scales_at + ntt_scale_index(arg(2), arg(3))));
    } else if (mode == "plan") {
        for (uint32_t k = NTT_MIN_K; k <= NTT_MAX_K; ++k) {
            std::printf("%u %u", k, ntt_passes(k));
            for (uint32_t p = 0; p < ntt_passes(k); ++p) std::printf(" %u:%u:%u", ntt_pass(k, p).s0, ntt_pass(k, p).m, ntt_pass(k, p).a);
            std::printf("\n");
        }
    } else if (mode == "sizes") {
        const NttTables t = ntt_tables(arg(2));
        std::printf("%llu %llu %u %u %u %u\n", (unsigned long long)ntt_tables_bytes(arg(2)), (unsigned long long)ntt_workspace_bytes(arg(3), arg(4)), t.low_at, t.high_at,
                    t.scales_at, t.cells);
    } else if (mode == "run" && argc == 9) {
        const std::string name = argv[2];
        const uint32_t k = arg(3), ext_k = arg(4), zeta_sel = arg(5), max_k = arg(6);
        const Tables t(max_k);
        const bool extended = name == "c2e" || name == "e2c";
        const uint32_t size_k = extended ? ext_k : k, src_k = name == "c2e" ? k : size_k;
        const std::vector<Fr> in = read_cells(argv[7], (size_t)1 << src_k);
        std::vector<Fr> out((size_t)1 << size_k);
        if (name == "l2c") transform(t, size_k, src_k, max_k, 0, F_INVERSE, F_SCALE, in, out);
        else if (name == "c2l") transform(t, size_k, src_k, max_k, 0, 0, 0, in, out);
        else if (name == "c2e") transform(t, size_k, src_k, max_k, zeta_sel, F_ZETA_LOAD, 0, in, out);
        else if (name == "e2c") transform(t, size_k, src_k, max_k, zeta_sel, F_INVERSE, F_SCALE | F_ZETA_STORE, in, out);
        else return 2;
        FILE *f = std::fopen(argv[8], "wb");
        if (!f || std::fwrite(out.data(), sizeof(Fr), out.size(), f) != out.size()) return 3;
        std::fclose(f);
    } else if (mode == "sparse" && argc >= 10) {
        const uint32_t k = arg(2), max_k = arg(3);
        const Tables t(max_k);
        std::vector<Fr> in((size_t)1 << k, FR_ZERO), out((size_t)1 << k);
        for (int j = 0; j < 3; ++j) in.at(arg(4 + 2 * j)) = parse_cell(argv[5 + 2 * j]);
        transform(t, k, k, max_k, 0, 0, 0, in, out);
        for (int i = 10; i < argc; ++i) print_cell(out.at(arg(i)));
    } else if (mode == "sparse_ext" && argc >= 12) {
        const uint32_t k = arg(2), ext_k = arg(3), zeta_sel = arg(4), max_k = arg(5);
        const Tables t(max_k);
        std::vector<Fr> in((size_t)1 << k, FR_ZERO), ext((size_t)1 << ext_k), back((size_t)1 << ext_k);
        for (int j = 0; j < 3; ++j) in.at(arg(6 + 2 * j)) = parse_cell(argv[7 + 2 * j]);
        transform(t, ext_k, k, max_k, zeta_sel, F_ZETA_LOAD, 0, in, ext);
        for (int i = 12; i < argc; ++i) print_cell(ext.at(arg(i)));
        transform(t, ext_k, ext_k, max_k, zeta_sel, F_INVERSE, F_SCALE | F_ZETA_STORE, ext, back);  // and back: the coefficients, then zeros
        size_t wrong = 0;
        for (size_t i = 0; i < back.size(); ++i) wrong += !fr_eq(back[i], i < in.size() ? in[i] : FR_ZERO);
        std::printf("%zu\n", wrong);
    } else if (mode == "positions" && argc == 6) {
        const NttPass q = ntt_pass(arg(2), arg(3));
        std::printf("%u %u\n", ntt_slot_position(q, arg(4), arg(5)), ntt_slot_twiddle(q, arg(4), arg(5)));
    } else {
        return 2;
    }
    return 0;
}
