// open_driver.cpp -- csrc/aesw_open.h alone under g++ (tests/test_open_model.py): the sizes as text, the serial recurrence, and the
// chunk / carry / scan decomposition of open/aesw_open.hip executed on the CPU through the header's own functions -- workgroup by
// workgroup, wave by wave and lane by lane, the workspace laid out as the header says -- with fr_mul and fr_add of aesw_fr.h.  A
// program of its own, so that it can be built under -fsanitize=address,undefined.
//   sizes K N_COLS N_POINTS                   workspace bytes, chunks, turns, the first chunk of every turn
//   constants                                 chunk, rows per lane, turn, powers per point, the five power indices
//   serial K COEFF POINT QUOT REM             one column by open_serial; files of 32-byte cells
//   evaluate K N_COLS N_POINTS COEFF POINTS EVALS      the powers, chunk and carry passes
//   divide K N_COLS COEFF POINT QUOT REM      the powers, chunk, carry and scan passes; QUOT may be COEFF's path (in place)
//   fold K N_COLS COEFF V ACC|- FOLDED        open_fold_step, column after column
//   check K SEED POINT_HEX                    a seeded column by both: the number of cells of q, rem and the value that differ
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_open.h"

using namespace aesw;

static Fr parse_cell(const char *hex) {
    Fr v = FR_ZERO;
    if (std::strlen(hex) != 64) std::exit(2);
    for (int i = 0; i < FR_LIMBS; ++i) v.l[FR_LIMBS - 1 - i] = (uint32_t)std::strtoul(std::string(hex + 8 * i, 8).c_str(), nullptr, 16);
    return v;
}
static std::vector<Fr> read_cells(const char *path, size_t cells) {
    std::vector<Fr> v(cells);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(Fr), cells, f) != cells) std::exit(3);
    std::fclose(f);
    return v;
}
static void write_cells(const char *path, const std::vector<Fr> &v) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(Fr), v.size(), f) != v.size()) std::exit(3);
    std::fclose(f);
}

typedef std::vector<Fr> Cells;

// open_wave_suffix of the kernels: 64 values, every step reads what the step before left
static void wave_suffix(Fr (&v)[OPEN_LANES], const Cells &ws, uint32_t point, uint32_t base) {
    for (uint32_t j = 0; (1u << j) < OPEN_LANES; ++j) {
        Fr next[OPEN_LANES];
        for (uint32_t l = 0; l < OPEN_LANES; ++l)
            next[l] = l + (1u << j) < OPEN_LANES ? open_join(v[l], ws.at(open_power_at(point, open_scan_power(base, j))), v[l + (1u << j)]) : v[l];
        std::memcpy(v, next, sizeof(next));
    }
}

static void powers_pass(Cells &ws, const Cells &points) {
    for (uint32_t p = 0; p < points.size(); ++p) {
        Fr v = points[p];
        for (uint32_t s = 0; s < OPEN_POWERS; ++s) {
            ws.at(open_power_at(p, s)) = v;
            v = fr_mul(v, v);
        }
    }
}

static void lane_cells(const Cells &coeff, uint32_t k, uint32_t column, uint32_t i0, Fr (&c)[OPEN_ROWS_PER_LANE]) {
    for (uint32_t q = 0; q < OPEN_ROWS_PER_LANE; ++q) c[q] = coeff.at(((uint64_t)column << k) + i0 + q);
}

static void chunk_pass(Cells &ws, const Cells &coeff, uint32_t k, uint32_t n_cols, uint32_t n_points) {
    for (uint32_t column = 0; column < n_cols; ++column)
        for (uint32_t chunk = 0; chunk < open_chunks(k); ++chunk)
            for (uint32_t pt = 0; pt < n_points; ++pt) {
                Fr total[OPEN_WAVES];
                for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                    Fr t[OPEN_LANES];
                    for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                        Fr c[OPEN_ROWS_PER_LANE], h[OPEN_ROWS_PER_LANE];
                        lane_cells(coeff, k, column, chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE, c);
                        open_lane_horner(c, ws.at(open_power_at(pt, OPEN_POWER_CELL)), h);
                        t[lane] = h[0];
                    }
                    wave_suffix(t, ws, pt, OPEN_POWER_LANE);
                    total[wave] = t[0];
                }
                ws.at(open_chunk_at(k, n_points, column, pt, chunk)) =
                    open_join_waves<OPEN_WAVES>(ws.at(open_power_at(pt, OPEN_POWER_WAVE)), FR_ZERO, [&](int w) { return total[w]; }, [](int, const Fr &) {});
            }
}

static void carry_pass(Cells &ws, uint32_t k, uint32_t n_cols, uint32_t n_points, Cells &out, bool write_carries) {
    const uint32_t chunks = open_chunks(k);
    for (uint32_t pair = 0; pair < n_cols * n_points; ++pair) {
        const uint32_t pt = pair % n_points;
        const uint64_t cells = open_chunk_at(k, n_points, pair / n_points, pt, 0);
        const auto power = [&](uint32_t s) { return ws.at(open_power_at(pt, s)); };
        Fr running = FR_ZERO;
        for (uint32_t t = 0; t < open_turns(k); ++t) {
            Fr incl[OPEN_WAVES][OPEN_LANES], above[OPEN_WAVES];
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    const uint32_t i = open_turn_first(k, t) + wave * OPEN_LANES + lane;
                    incl[wave][lane] = i < chunks ? ws.at(cells + i) : FR_ZERO;
                }
                wave_suffix(incl[wave], ws, pt, OPEN_POWER_CHUNK);
            }
            running = open_join_waves<OPEN_WAVES>(power(OPEN_POWER_CHUNK_WAVE), running, [&](int w) { return incl[w][0]; }, [&](int w, const Fr &a) { above[w] = a; });
            if (!write_carries) continue;
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                Fr here[OPEN_LANES];
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) here[lane] = open_join(incl[wave][lane], open_lane_weight(OPEN_POWER_CHUNK, lane, power), above[wave]);
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    const uint32_t i = open_turn_first(k, t) + wave * OPEN_LANES + lane;
                    if (i < chunks) ws.at(cells + i) = lane == OPEN_LANES - 1 ? above[wave] : here[lane + 1];
                }
            }
        }
        out.at(pair) = running;
    }
}

// quot may be coeff: a lane reads its cells before it writes them
static void scan_pass(const Cells &ws, const Cells &coeff, Cells &quot, uint32_t k, uint32_t n_cols) {
    const auto power = [&](uint32_t s) { return ws.at(open_power_at(0, s)); };
    const Fr z = power(OPEN_POWER_CELL);
    for (uint32_t column = 0; column < n_cols; ++column)
        for (uint32_t chunk = 0; chunk < open_chunks(k); ++chunk) {
            Fr c[OPEN_WAVES][OPEN_LANES][OPEN_ROWS_PER_LANE], incl[OPEN_WAVES][OPEN_LANES], above[OPEN_WAVES];
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    Fr h[OPEN_ROWS_PER_LANE];
                    lane_cells(coeff, k, column, chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE, c[wave][lane]);
                    open_lane_horner(c[wave][lane], z, h);
                    incl[wave][lane] = h[0];
                }
                wave_suffix(incl[wave], ws, 0, OPEN_POWER_LANE);
            }
            open_join_waves<OPEN_WAVES>(power(OPEN_POWER_WAVE), ws.at(open_chunk_at(k, 1, column, 0, chunk)), [&](int w) { return incl[w][0]; },
                                        [&](int w, const Fr &a) { above[w] = a; });
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                Fr here[OPEN_LANES];
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) here[lane] = open_join(incl[wave][lane], open_lane_weight(OPEN_POWER_LANE, lane, power), above[wave]);
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    Fr q[OPEN_ROWS_PER_LANE];
                    open_lane_quotient(c[wave][lane], z, lane == OPEN_LANES - 1 ? above[wave] : here[lane + 1], q);
                    for (uint32_t j = 0; j < OPEN_ROWS_PER_LANE; ++j)
                        quot.at(((uint64_t)column << k) + chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE + j) = q[j];
                }
            }
        }
}

static Cells evaluate(const Cells &coeff, const Cells &points, uint32_t k, uint32_t n_cols) {
    const uint32_t n_points = (uint32_t)points.size();
    Cells ws(open_workspace_cells(k, n_cols, n_points)), evals((size_t)n_cols * n_points);
    if (ws.size() * sizeof(Fr) != open_workspace_bytes(k, n_cols, n_points)) std::exit(4);
    powers_pass(ws, points);
    chunk_pass(ws, coeff, k, n_cols, n_points);
    carry_pass(ws, k, n_cols, n_points, evals, false);
    return evals;
}

static Cells divide(const Cells &coeff, Cells &quot, const Fr &point, uint32_t k, uint32_t n_cols) {
    Cells ws(open_workspace_cells(k, n_cols, 1)), rem(n_cols);
    powers_pass(ws, Cells(1, point));
    chunk_pass(ws, coeff, k, n_cols, 1);
    carry_pass(ws, k, n_cols, 1, rem, true);
    scan_pass(ws, coeff, quot, k, n_cols);
    return rem;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const auto arg = [&](int i) { return i < argc ? (uint32_t)std::strtoul(argv[i], nullptr, 10) : 0u; };
    if (mode == "sizes" && argc == 5) {
        const uint32_t k = arg(2);
        std::printf("%llu %u %u", (unsigned long long)open_workspace_bytes(k, arg(3), arg(4)), open_k_ok(k) ? open_chunks(k) : 0u, open_k_ok(k) ? open_turns(k) : 0u);
        for (uint32_t t = 0; open_k_ok(k) && t < open_turns(k) && t < 4; ++t) std::printf(" %u", open_turn_first(k, t));
        std::printf("\n");
    } else if (mode == "constants") {
        std::printf("%u %u %u %u %u %u %u %u %u\n", OPEN_CHUNK, OPEN_ROWS_PER_LANE, OPEN_TURN, OPEN_POWERS, OPEN_POWER_CELL, OPEN_POWER_LANE, OPEN_POWER_WAVE, OPEN_POWER_CHUNK,
                    OPEN_POWER_CHUNK_WAVE);
    } else if (mode == "serial" && argc == 7) {
        const uint32_t k = arg(2);
        const Cells coeff = read_cells(argv[3], (size_t)1 << k), point = read_cells(argv[4], 1);
        Cells quot((size_t)1 << k);
        const Fr rem = open_serial((uint64_t)1 << k, point[0], FR_ZERO, [&](uint64_t i) { return coeff[i]; }, [&](uint64_t i, const Fr &s) { if (i) quot.at(i - 1) = s; });
        quot.back() = FR_ZERO;
        write_cells(argv[5], quot);
        write_cells(argv[6], Cells(1, rem));
    } else if (mode == "evaluate" && argc == 8) {
        const uint32_t k = arg(2), n_cols = arg(3), n_points = arg(4);
        write_cells(argv[7], evaluate(read_cells(argv[5], (size_t)n_cols << k), read_cells(argv[6], n_points), k, n_cols));
    } else if (mode == "divide" && argc == 8) {
        const uint32_t k = arg(2), n_cols = arg(3);
        Cells coeff = read_cells(argv[4], (size_t)n_cols << k);
        const Fr point = read_cells(argv[5], 1)[0];
        if (std::string(argv[6]) == argv[4]) {  // in place
            const Cells rem = divide(coeff, coeff, point, k, n_cols);
            write_cells(argv[6], coeff);
            write_cells(argv[7], rem);
        } else {
            Cells quot(coeff.size());
            write_cells(argv[7], divide(coeff, quot, point, k, n_cols));
            write_cells(argv[6], quot);
        }
    } else if (mode == "fold" && argc == 8) {
        const uint32_t k = arg(2), n_cols = arg(3);
        const Cells coeff = read_cells(argv[4], (size_t)n_cols << k);
        const Fr v = read_cells(argv[5], 1)[0];
        Cells acc = std::string(argv[6]) == "-" ? Cells((size_t)1 << k, FR_ZERO) : read_cells(argv[6], (size_t)1 << k);
        for (uint32_t c = 0; c < n_cols; ++c)
            for (size_t i = 0; i < acc.size(); ++i) acc[i] = open_fold_step(acc[i], v, coeff.at(((size_t)c << k) + i));
        write_cells(argv[7], acc);
    } else if (mode == "check" && argc == 5) {
        const uint32_t k = arg(2);
        const Fr point = parse_cell(argv[4]);
        Cells coeff((size_t)1 << k), quot((size_t)1 << k), serial((size_t)1 << k, FR_ZERO);
        uint64_t x = 0x2545f4914f6cdd1dull + arg(3);
        for (Fr &c : coeff) {  // seeded canonical cells: the top limb stays below r's
            for (int i = 0; i < FR_LIMBS; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c.l[i] = (uint32_t)(x >> 16); }
            c.l[FR_LIMBS - 1] &= 0x1fffffffu;
        }
        const Fr rem = open_serial((uint64_t)1 << k, point, FR_ZERO, [&](uint64_t i) { return coeff[i]; }, [&](uint64_t i, const Fr &s) { if (i) serial.at(i - 1) = s; });
        const Fr value = evaluate(coeff, Cells(1, point), k, 1).at(0);
        const Fr rem2 = divide(coeff, quot, point, k, 1).at(0);
        size_t wrong = !fr_eq(rem, value) + !fr_eq(rem, rem2);
        for (size_t i = 0; i < quot.size(); ++i) wrong += !fr_eq(quot[i], serial[i]);
        std::printf("%zu\n", wrong);
    } else {
        return 2;
    }
    return 0;
}
