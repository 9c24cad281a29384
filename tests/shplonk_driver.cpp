// shplonk_driver.cpp -- csrc/aesw_shplonk.h (over aesw_open.h and aesw_fr.h) alone under g++ (tests/test_shplonk_model.py): the
// sizes as text, and the kernels of shplonk/aesw_shplonk.hip executed on the CPU through the header's own functions -- the small
// phases thread by thread, the chunk / carry / scan passes of a set's quotient workgroup by workgroup, wave by wave and lane by
// lane, the scalars block and the workspace laid out as the headers say.  A program of its own, so that it can be built under
// -fsanitize=address,undefined.
//   constants                     the cell of every table of the scalars block, in the order of the table ids; then the report's bytes
//   sizes N_SETS MAX_COLS K       scalars bytes, workspace bytes
//   plan PLAN                     0 for a plan that is taken, 1 and the reason for one that is refused
//   stage K PLAN CELLS OUT        the whole stage.  PLAN: text, "n_points n_sets" then per set "t m idx...".  CELLS: the points, y, v, u,
//                                 the evaluations, then the columns set by set.  OUT: the scalars block after both phases, then per set
//                                 N_i and its 8 remainder cells (those past t_i zero), then h, L' and W, then the report (two cells).
//   check K SEED T                a seeded numerator at T seeded points by the passes against sum_s w_s S^(s) of open_serial: the
//                                 number of cells of the quotient and of remainders that differ
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_shplonk.h"

using namespace aesw;

typedef std::vector<Fr> Cells;

static Cells read_cells(FILE *f, size_t cells) {
    Cells v(cells);
    if (cells && std::fread(v.data(), sizeof(Fr), cells, f) != cells) std::exit(3);
    return v;
}
static void write_cells(FILE *f, const Cells &v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(Fr), v.size(), f) != v.size()) std::exit(3);
}

struct HostPlan {
    uint32_t n_points = 0, n_sets = 0;
    std::vector<uint32_t> t, m, index;
};
static HostPlan read_plan(const char *path) {
    HostPlan p;
    FILE *f = std::fopen(path, "r");
    if (!f || std::fscanf(f, "%u %u", &p.n_points, &p.n_sets) != 2 || p.n_sets > 64) std::exit(3);
    for (uint32_t i = 0; i < p.n_sets; ++i) {
        uint32_t t, m;
        if (std::fscanf(f, "%u %u", &t, &m) != 2 || t > 64) std::exit(3);
        p.t.push_back(t);
        p.m.push_back(m);
        for (uint32_t s = 0; s < t; ++s) {
            uint32_t x;
            if (std::fscanf(f, "%u", &x) != 1) std::exit(3);
            p.index.push_back(x);
        }
    }
    std::fclose(f);
    return p;
}

// the scalars block: cells, with the plan's words at its front
struct Block {
    Cells cells;
    uint32_t word(uint32_t i) const { uint32_t w; std::memcpy(&w, reinterpret_cast<const uint8_t *>(cells.data()) + 4 * i, 4); return w; }
    void set_word(uint32_t i, uint32_t w) { std::memcpy(reinterpret_cast<uint8_t *>(cells.data()) + 4 * i, &w, 4); }
    uint32_t sets() const { return shplonk_clamp(word(SHPLONK_PLAN_N_SETS), SHPLONK_MAX_SETS); }
    uint32_t t(uint32_t set) const { return shplonk_clamp(word(SHPLONK_PLAN_T + set), SHPLONK_MAX_SET_POINTS); }
    uint32_t index(uint32_t set, uint32_t s) const { return word(SHPLONK_PLAN_INDEX + SHPLONK_MAX_SET_POINTS * set + s) & (SHPLONK_MAX_POINTS - 1); }
};

// shplonk_prepare_kernel, thread by thread
static void prepare(const ShplonkPlan &plan, const Cells &points, const Cells &evals, const Fr &y, const Fr &v, Block &b, uint64_t (&report)[SHPLONK_REPORT_WORDS]) {
    const uint32_t n_sets = plan.w[SHPLONK_PLAN_N_SETS], max_cols = plan.w[SHPLONK_PLAN_MAX_COLS];
    Fr scaled[SHPLONK_MAX_SETS][SHPLONK_MAX_SET_POINTS], zc[SHPLONK_MAX_SETS][SHPLONK_MAX_SET_POINTS + 1], out[SHPLONK_MAX_SETS][SHPLONK_MAX_SET_POINTS];
    uint64_t zeros = 0;
    for (uint32_t tid = 0; tid < SHPLONK_PLAN_WORDS; ++tid) b.set_word(tid, plan.w[tid]);
    for (uint32_t j = 0; j < max_cols; ++j) b.cells.at(SHPLONK_AT_Y_POW + j) = shplonk_pow(y, j);
    for (uint32_t tid = 0; tid < SHPLONK_MAX_SETS; ++tid) b.cells.at(SHPLONK_AT_V_POW + tid) = tid < n_sets ? shplonk_pow(v, tid) : FR_ZERO;
    for (uint32_t tid = 0; tid < SHPLONK_MAX_SETS * SHPLONK_MAX_SET_POINTS; ++tid) {
        const uint32_t i = tid / SHPLONK_MAX_SET_POINTS, s = tid % SHPLONK_MAX_SET_POINTS, t = i < n_sets ? plan.w[SHPLONK_PLAN_T + i] : 0u;
        Fr ebar = FR_ZERO, w = FR_ZERO, vw = FR_ZERO;
        uint32_t zero = 0;
        if (s < t) {
            const uint32_t m = plan.w[SHPLONK_PLAN_M + i], first = plan.w[SHPLONK_PLAN_EVAL + i];
            ebar = shplonk_horner(m, y, [&](uint32_t j) { return evals.at(first + (size_t)j * t + s); });
            w = shplonk_weight(t, s, [&](uint32_t r) { return points.at(plan.w[SHPLONK_PLAN_INDEX + SHPLONK_MAX_SET_POINTS * i + r]); }, zero);
            vw = fr_mul(shplonk_pow(v, i), w);
        }
        scaled[i][s] = fr_mul(ebar, w);
        zeros += zero;
        b.cells.at(SHPLONK_AT_EBAR + tid) = ebar;
        b.cells.at(SHPLONK_AT_W + tid) = w;
        b.cells.at(SHPLONK_AT_VW + tid) = vw;
    }
    for (uint32_t i = 0; i < SHPLONK_MAX_SETS; ++i) {
        const uint32_t t = i < n_sets ? plan.w[SHPLONK_PLAN_T + i] : 0u;
        shplonk_neg_interpolant(
            t, [&](uint32_t r) { return points.at(plan.w[SHPLONK_PLAN_INDEX + SHPLONK_MAX_SET_POINTS * i + r]); }, [&](uint32_t s) { return scaled[i][s]; },
            [&](uint32_t r) -> Fr & { return zc[i][r]; }, [&](uint32_t d) -> Fr & { return out[i][d]; });
        for (uint32_t d = 0; d < SHPLONK_MAX_SET_POINTS; ++d) b.cells.at(SHPLONK_AT_NEG_R + SHPLONK_MAX_SET_POINTS * i + d) = d < t ? out[i][d] : FR_ZERO;
    }
    for (uint32_t word = 0; word < SHPLONK_REPORT_WORDS; ++word) report[word] = (SHPLONK_REP_NONE_MASK >> word & 1u) ? ~0ull : 0ull;
    report[SHPLONK_REP_ZERO_DIFFS] = zeros;
}

// shplonk_finish_kernel, thread by thread
static void finish(const Cells &points, const Fr &u, Block &b, uint64_t (&report)[SHPLONK_REPORT_WORDS]) {
    const uint32_t n_sets = b.sets(), n_points = shplonk_clamp(b.word(SHPLONK_PLAN_N_POINTS), SHPLONK_MAX_POINTS);
    Fr z[SHPLONK_MAX_SETS + 1], r_u[SHPLONK_MAX_SETS + 1], coef[SHPLONK_MAX_SETS + 1], term[SHPLONK_MAX_SETS], z0_inv = FR_ZERO;
    for (uint32_t tid = 0; tid <= SHPLONK_MAX_SETS; ++tid) {
        z[tid] = r_u[tid] = FR_ZERO;
        if (tid <= n_sets) z[tid] = shplonk_vanish(n_points, tid < n_sets ? b.word(SHPLONK_PLAN_MASK + tid) : 0u, u, [&](uint32_t p) { return points.at(p); });
        if (tid < n_sets) r_u[tid] = fr_sub(FR_ZERO, shplonk_horner(b.t(tid), u, [&](uint32_t d) { return b.cells.at(SHPLONK_AT_NEG_R + SHPLONK_MAX_SET_POINTS * tid + d); }));
        if (tid == 0) {
            z0_inv = fr_inv(z[0]);
            b.cells.at(SHPLONK_AT_Z0_INV) = z0_inv;
            report[SHPLONK_REP_Z0_ZERO] = fr_is_zero(z[0]) ? 1 : 0;
        }
    }
    for (uint32_t tid = 0; tid <= SHPLONK_MAX_SETS; ++tid) {
        Fr c = FR_ZERO;
        if (tid <= n_sets) c = fr_mul(z0_inv, z[tid]);
        if (tid < n_sets) c = fr_mul(c, b.cells.at(SHPLONK_AT_V_POW + tid));
        if (tid == n_sets) c = fr_sub(FR_ZERO, c);
        coef[tid] = c;
        b.cells.at(SHPLONK_AT_L_COEF + tid) = c;
        if (tid < SHPLONK_MAX_SETS) {
            term[tid] = fr_mul(c, r_u[tid]);
            b.cells.at(SHPLONK_AT_Z + tid) = tid < n_sets ? z[tid] : FR_ZERO;
        }
        if (tid == n_sets) b.cells.at(SHPLONK_AT_Z_T) = z[tid];
    }
    for (uint32_t tid = 0; tid < SHPLONK_MAX_LOW; ++tid) {
        Fr low = FR_ZERO;
        for (uint32_t i = 0; i < n_sets; ++i) low = fr_sub(low, fr_mul(coef[i], b.cells.at(SHPLONK_AT_NEG_R + SHPLONK_MAX_SET_POINTS * i + tid)));
        if (tid == 0) {
            Fr constant = FR_ZERO;
            for (uint32_t i = 0; i < n_sets; ++i) constant = fr_sub(constant, term[i]);
            b.cells.at(SHPLONK_AT_L_CONST) = constant;
            low = fr_add(low, constant);
        }
        b.cells.at(SHPLONK_AT_L_LOW + tid) = low;
    }
}

// shplonk_combine_kernel, cell by cell; out may be acc
static void combine(uint32_t k, uint32_t n_cols, const Fr *coeff, const Fr *coefs, const Fr *low, uint32_t n_low, const Fr *acc, Fr *out) {
    for (uint32_t i = 0; i < 1u << k; ++i) {
        Fr a = acc ? acc[i] : FR_ZERO;
        if (i < n_low) a = fr_add(a, low[i]);
        out[i] = shplonk_combine_cell(a, n_cols, [&](uint32_t j) { return coefs[j]; }, [&](uint32_t j) { return coeff[((size_t)j << k) + i]; });
    }
}

// open_wave_suffix of the kernels: 64 values, every step reads what the step before left
static void wave_suffix(Fr (&v)[OPEN_LANES], const Cells &ws, uint32_t point, uint32_t base) {
    for (uint32_t j = 0; (1u << j) < OPEN_LANES; ++j) {
        Fr next[OPEN_LANES];
        for (uint32_t l = 0; l < OPEN_LANES; ++l)
            next[l] = l + (1u << j) < OPEN_LANES ? open_join(v[l], ws.at(open_power_at(point, open_scan_power(base, j))), v[l + (1u << j)]) : v[l];
        std::memcpy(v, next, sizeof(next));
    }
}
static void lane_cells(const Fr *column, uint32_t i0, Fr (&c)[OPEN_ROWS_PER_LANE]) {
    for (uint32_t q = 0; q < OPEN_ROWS_PER_LANE; ++q) c[q] = column[i0 + q];
}

// the five kernels of aesw_shplonk_quotient_device; out may be numer or acc; rem: 8 cells
static void quotient(uint32_t k, uint32_t set, const Fr *numer, const Cells &points, const Block &b, const Fr *acc, Fr *out, Fr *rem, uint64_t (&report)[SHPLONK_REPORT_WORDS]) {
    const uint32_t t = b.t(set), chunks = open_chunks(k), P = SHPLONK_WS_POINTS;
    Cells ws(shplonk_workspace_bytes(k) / sizeof(Fr));
    for (uint32_t s = 0; s < t; ++s) {  // the powers
        Fr z = points.at(b.index(set, s));
        for (uint32_t e = 0; e < OPEN_POWERS; ++e) {
            ws.at(open_power_at(s, e)) = z;
            z = fr_mul(z, z);
        }
    }
    for (uint32_t chunk = 0; chunk < chunks; ++chunk)  // the chunk pass
        for (uint32_t pt = 0; pt < t; ++pt) {
            Fr total[OPEN_WAVES];
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                Fr v[OPEN_LANES];
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    Fr c[OPEN_ROWS_PER_LANE], h[OPEN_ROWS_PER_LANE];
                    lane_cells(numer, chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE, c);
                    open_lane_horner(c, ws.at(open_power_at(pt, OPEN_POWER_CELL)), h);
                    v[lane] = h[0];
                }
                wave_suffix(v, ws, pt, OPEN_POWER_LANE);
                total[wave] = v[0];
            }
            ws.at(open_chunk_at(k, P, 0, pt, chunk)) =
                open_join_waves<OPEN_WAVES>(ws.at(open_power_at(pt, OPEN_POWER_WAVE)), FR_ZERO, [&](int w) { return total[w]; }, [](int, const Fr &) {});
        }
    for (uint32_t pt = 0; pt < t; ++pt) {  // the carry pass
        const uint64_t cells = open_chunk_at(k, P, 0, pt, 0);
        const auto power = [&](uint32_t s) { return ws.at(open_power_at(pt, s)); };
        Fr running = FR_ZERO;
        for (uint32_t turn = 0; turn < open_turns(k); ++turn) {
            Fr incl[OPEN_WAVES][OPEN_LANES], above[OPEN_WAVES];
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    const uint32_t i = open_turn_first(k, turn) + wave * OPEN_LANES + lane;
                    incl[wave][lane] = i < chunks ? ws.at(cells + i) : FR_ZERO;
                }
                wave_suffix(incl[wave], ws, pt, OPEN_POWER_CHUNK);
            }
            running = open_join_waves<OPEN_WAVES>(power(OPEN_POWER_CHUNK_WAVE), running, [&](int w) { return incl[w][0]; }, [&](int w, const Fr &a) { above[w] = a; });
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                Fr here[OPEN_LANES];
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) here[lane] = open_join(incl[wave][lane], open_lane_weight(OPEN_POWER_CHUNK, lane, power), above[wave]);
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    const uint32_t i = open_turn_first(k, turn) + wave * OPEN_LANES + lane;
                    if (i < chunks) ws.at(cells + i) = lane == OPEN_LANES - 1 ? above[wave] : here[lane + 1];
                }
            }
        }
        rem[pt] = running;
    }
    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {  // the scan pass: every lane reads before any lane of the chunk writes, and a lane only its own cells
        static Fr c[OPEN_WAVES][OPEN_LANES][OPEN_ROWS_PER_LANE], o[OPEN_WAVES][OPEN_LANES][OPEN_ROWS_PER_LANE];
        for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave)
            for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                const uint32_t i0 = chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE;
                lane_cells(numer, i0, c[wave][lane]);
                if (acc) lane_cells(acc, i0, o[wave][lane]);
                else for (Fr &x : o[wave][lane]) x = FR_ZERO;
            }
        for (uint32_t pt = 0; pt < t; ++pt) {
            const auto power = [&](uint32_t s) { return ws.at(open_power_at(pt, s)); };
            const Fr z = power(OPEN_POWER_CELL), scale = b.cells.at(SHPLONK_AT_VW + SHPLONK_MAX_SET_POINTS * set + pt);
            Fr incl[OPEN_WAVES][OPEN_LANES], above[OPEN_WAVES];
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) {
                    Fr h[OPEN_ROWS_PER_LANE];
                    open_lane_horner(c[wave][lane], z, h);
                    incl[wave][lane] = h[0];
                }
                wave_suffix(incl[wave], ws, pt, OPEN_POWER_LANE);
            }
            open_join_waves<OPEN_WAVES>(power(OPEN_POWER_WAVE), ws.at(open_chunk_at(k, P, 0, pt, chunk)), [&](int w) { return incl[w][0]; }, [&](int w, const Fr &a) { above[w] = a; });
            for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave) {
                Fr here[OPEN_LANES];
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane) here[lane] = open_join(incl[wave][lane], open_lane_weight(OPEN_POWER_LANE, lane, power), above[wave]);
                for (uint32_t lane = 0; lane < OPEN_LANES; ++lane)
                    shplonk_lane_accumulate(c[wave][lane], z, lane == OPEN_LANES - 1 ? above[wave] : here[lane + 1], scale, o[wave][lane]);
            }
        }
        for (uint32_t wave = 0; wave < OPEN_WAVES; ++wave)
            for (uint32_t lane = 0; lane < OPEN_LANES; ++lane)
                for (uint32_t j = 0; j < OPEN_ROWS_PER_LANE; ++j) out[chunk * OPEN_CHUNK + (wave * OPEN_LANES + lane) * OPEN_ROWS_PER_LANE + j] = o[wave][lane][j];
    }
    bool any = false;  // the report kernel
    for (uint32_t s = 0; s < t; ++s) any |= !fr_is_zero(rem[s]);
    if (any) {
        report[SHPLONK_REP_BAD_SETS] += 1;
        if (set < report[SHPLONK_REP_FIRST_BAD]) report[SHPLONK_REP_FIRST_BAD] = set;
    }
}

static Fr seeded(uint64_t &x) {  // a canonical cell: the top limb stays below r's
    Fr c;
    for (int i = 0; i < FR_LIMBS; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c.l[i] = (uint32_t)(x >> 16); }
    c.l[FR_LIMBS - 1] &= 0x1fffffffu;
    return c;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const auto arg = [&](int i) { return i < argc ? (uint32_t)std::strtoul(argv[i], nullptr, 10) : 0u; };
    if (mode == "constants") {
        for (uint32_t table = 0; table < SHPLONK_TABLES; ++table) std::printf("%llu ", (unsigned long long)shplonk_table_at(table, 0));
        std::printf("%u\n", SHPLONK_REPORT_BYTES);
    } else if (mode == "sizes" && argc == 5) {
        std::printf("%llu %llu\n", (unsigned long long)shplonk_scalars_bytes(arg(2), arg(3)), (unsigned long long)shplonk_workspace_bytes(arg(4)));
    } else if (mode == "plan" && argc == 3) {
        const HostPlan hp = read_plan(argv[2]);
        ShplonkPlan plan;
        const char *why = shplonk_plan_fill(hp.n_points, hp.n_sets, hp.t.data(), hp.m.data(), hp.index.data(), plan);
        std::printf("%d %s\n", why ? 1 : 0, why ? why : "");
    } else if (mode == "stage" && argc == 6) {
        const uint32_t k = arg(2);
        const size_t n = (size_t)1 << k;
        const HostPlan hp = read_plan(argv[3]);
        ShplonkPlan plan;
        if (!open_k_ok(k) || shplonk_plan_fill(hp.n_points, hp.n_sets, hp.t.data(), hp.m.data(), hp.index.data(), plan)) return 4;
        FILE *in = std::fopen(argv[4], "rb");
        if (!in) return 3;
        const Cells points = read_cells(in, hp.n_points), yvu = read_cells(in, 3), evals = read_cells(in, shplonk_plan_evals(plan));
        Block b;
        b.cells.assign(shplonk_scalars_bytes(hp.n_sets, plan.w[SHPLONK_PLAN_MAX_COLS]) / sizeof(Fr), FR_ZERO);
        uint64_t report[SHPLONK_REPORT_WORDS];
        prepare(plan, points, evals, yvu[0], yvu[1], b, report);
        Cells work((hp.n_sets + 1) * n), rems((size_t)hp.n_sets * SHPLONK_MAX_SET_POINTS, FR_ZERO), line(n);
        Fr *h = work.data() + hp.n_sets * n;
        for (uint32_t i = 0; i < hp.n_sets; ++i) {
            const Cells columns = read_cells(in, hp.m[i] * n);
            combine(k, hp.m[i], columns.data(), &b.cells.at(SHPLONK_AT_Y_POW), &b.cells.at(SHPLONK_AT_NEG_R + SHPLONK_MAX_SET_POINTS * i), hp.t[i], nullptr, work.data() + i * n);
            quotient(k, i, work.data() + i * n, points, b, i ? h : nullptr, h, rems.data() + (size_t)i * SHPLONK_MAX_SET_POINTS, report);  // h accumulates in place
        }
        std::fclose(in);
        finish(points, yvu[2], b, report);
        combine(k, hp.n_sets + 1, work.data(), &b.cells.at(SHPLONK_AT_L_COEF), &b.cells.at(SHPLONK_AT_L_LOW), SHPLONK_MAX_LOW, nullptr, line.data());
        Cells w(n, FR_ZERO);  // the last division is aesw_open.h's, at one point: its serial form
        const Fr last = open_serial(n, yvu[2], FR_ZERO, [&](uint64_t i) { return line[i]; }, [&](uint64_t i, const Fr &s) { if (i) w.at(i - 1) = s; });
        std::memcpy(&report[SHPLONK_REP_LAST_REM], &last, sizeof(Fr));
        FILE *out = std::fopen(argv[5], "wb");
        if (!out) return 3;
        write_cells(out, b.cells);
        for (uint32_t i = 0; i < hp.n_sets; ++i) {
            write_cells(out, Cells(work.begin() + i * n, work.begin() + (i + 1) * n));
            write_cells(out, Cells(rems.begin() + (size_t)i * SHPLONK_MAX_SET_POINTS, rems.begin() + (size_t)(i + 1) * SHPLONK_MAX_SET_POINTS));
        }
        write_cells(out, Cells(h, h + n));
        write_cells(out, line);
        write_cells(out, w);
        if (std::fwrite(report, 8, SHPLONK_REPORT_WORDS, out) != SHPLONK_REPORT_WORDS) return 3;
        std::fclose(out);
    } else if (mode == "check" && argc == 5) {
        const uint32_t k = arg(2), t = arg(4);
        if (!open_k_ok(k) || !shplonk_set_points_ok(t)) return 4;
        const size_t n = (size_t)1 << k;
        uint64_t x = 0x2545f4914f6cdd1dull + arg(3);
        Cells numer(n), points(t), out(n), serial(n, FR_ZERO), rem(SHPLONK_MAX_SET_POINTS, FR_ZERO);
        for (Fr &c : numer) c = seeded(x);
        for (Fr &c : points) c = seeded(x);
        Block b;
        b.cells.assign(shplonk_scalars_bytes(1, 1) / sizeof(Fr), FR_ZERO);
        b.set_word(SHPLONK_PLAN_N_POINTS, t);
        b.set_word(SHPLONK_PLAN_N_SETS, 1);
        b.set_word(SHPLONK_PLAN_T, t);
        size_t wrong = 0;
        for (uint32_t s = 0; s < t; ++s) {
            uint32_t zero = 0;
            b.set_word(SHPLONK_PLAN_INDEX + s, s);
            const Fr w = shplonk_weight(t, s, [&](uint32_t r) { return points[r]; }, zero);
            b.cells.at(SHPLONK_AT_VW + s) = w;  // v^0 w_s
            const Fr value = open_serial(n, points[s], FR_ZERO, [&](uint64_t i) { return numer[i]; },
                                         [&](uint64_t i, const Fr &S) { if (i) serial[i - 1] = fr_add(serial[i - 1], fr_mul(w, S)); });
            rem[s] = value;  // held against the passes' below
        }
        uint64_t report[SHPLONK_REPORT_WORDS] = {0, ~0ull, 0, 0, 0, 0, 0, 0};
        Cells got(SHPLONK_MAX_SET_POINTS, FR_ZERO);
        quotient(k, 0, numer.data(), points, b, nullptr, out.data(), got.data(), report);
        for (uint32_t s = 0; s < t; ++s) wrong += !fr_eq(got[s], rem[s]);
        for (size_t i = 0; i < n; ++i) wrong += !fr_eq(out[i], serial[i]);
        std::printf("%zu\n", wrong);
    } else {
        return 2;
    }
    return 0;
}
