"""The specification of libaesw_shplonk.so without a GPU.

tests/shplonk_model.py states SHPLONK's multi-opening twice in Python integers -- as halo2 writes it (per column R_ij by Lagrange,
P_ij - R_ij, the fold under y, div_by_vanishing as successive divisions) and by partial fractions (what the device computes) -- and
is held against itself: the two are equal whenever the evaluations are the columns' own, Q_i Z_i == N_i, L(u) == 0 and
W (X - u) z_0 == L; with one evaluation changed the partial form is what the device is to give and the report names the set.
csrc/aesw_shplonk.h -- the plan, the scalars block, the report, what a thread of the small phases and a lane of the scan pass
compute -- is compiled alone with g++ into tests/shplonk_driver.cpp, which runs the kernels of shplonk/aesw_shplonk.hip on the CPU
through those functions and is held against the model cell for cell at k = 10 (one chunk) and k = 11 (the carry is crossed), with
t = 1, 2, 3 and 8, m = 1 and 5, at the points 0, 1, omega_k, r - 1 and seeded ones, once plain and once under
-fsanitize=address,undefined, and at k = 10 over sc.FULL_SETS, the 16 sets over 16 points the kernels are written for, with u
on a super-set point and with y, v and u at 0 and 1; at k = 19 (the carry's second turn) the driver holds the passes against the header's serial recurrence.
multiopen_plan is pure Python and is held here too."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ntt_model as nm
import open_model as om
import shplonk_cases as sc
import shplonk_model as sm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
R = nm.R


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("shplonk_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("shplonk_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "shplonk_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_shplonk.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text
    assert '#include "aesw_fr.h"' in text and '#include "aesw_open.h"' in text and text.count("#include \"aesw") == 2 and "NOT PINNED" in text


def small_stage(n, sets, wrong=None, seed=0):
    """sc.stage's shape over columns of n cells, the points of k = 10"""
    p, pts = sc.plan(sets), sc.points(10, seed)
    columns = [[nm.seeded_values(n, 0x736d + 16 * i + j + seed) for j in range(len(cols))] for i, (_idx, cols) in enumerate(p.sets)]
    evals = [[[om.evaluate(column, pts[q]) for q in idx] for column in columns[i]] for i, (idx, _cols) in enumerate(p.sets)]
    if wrong is not None:
        i, j, s = wrong
        evals[i][j][s] = (evals[i][j][s] + 1) % R
    return (p, pts, columns, evals) + tuple(nm.seeded_values(3, 0x79 + seed))


def vanishing(pts):
    z = [1]
    for point in pts:
        z = [((z[d - 1] if d else 0) - point * (z[d] if d < len(z) else 0)) % R for d in range(len(z) + 1)]
    return z


def times(a, b, n):
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if y:
                    assert i + j < n
                    out[i + j] = (out[i + j] + x * y) % R
    return out


@pytest.mark.parametrize("n", (16, 64))
def test_the_two_forms_are_equal_when_the_evaluations_are_the_columns_own(n):
    p, pts, columns, evals, y, v, u = small_stage(n, sc.SETS, seed=n)
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    h = [0] * n
    for i, (idx, _cols) in enumerate(p.sets):
        of_set, s = [pts[q] for q in idx], o["prep"]["sets"][i]
        q_halo2 = sm.halo2_quotient(columns[i], evals[i], of_set, y)
        q_partial, rems = sm.partial_quotient(o["numer"][i], of_set)
        assert q_halo2 == q_partial and rems == o["rems"][i] == [0] * len(idx) and any(q_partial)
        assert [-c % R for c in s["neg_r"]] == sm.lagrange(of_set, s["ebar"])  # the interpolant, by the weights and by Lagrange
        assert times(q_partial, vanishing(of_set), n) == o["numer"][i]  # Q_i Z_i == N_i
        h = [(a + pow(v, i, R) * c) % R for a, c in zip(h, q_partial)]
    assert h == o["h"] and o["report"] == dict(bad_sets=0, first_bad_set=None, zero_differences=0, z0_zero=0, last_remainder=0)
    # L as the rule writes it, from N^P_i and R_i(u); L(u) == 0 and W (X - u) z_0 == L
    fin, line = o["fin"], [0] * n
    for i, s in enumerate(o["prep"]["sets"]):
        np_i = sm.combine(columns[i], o["prep"]["y_pow"])
        r_u = om.evaluate(sm.lagrange(s["pts"], s["ebar"]), u)
        line = [(a + pow(v, i, R) * fin["z"][i] * ((c - r_u) % R if d == 0 else c)) % R for d, (a, c) in enumerate(zip(line, np_i))]
    line = [(a - fin["z_t"] * c) % R for a, c in zip(line, o["h"])]
    assert om.evaluate(line, u) == 0 and fin["z"][0] and fin["z0_inv"] * fin["z"][0] % R == 1
    assert [fin["z0_inv"] * c % R for c in line] == o["line"]
    assert [fin["z"][0] * c % R for c in om.times_linear(o["w"], u, 0)] == line
    assert fin["l_const"] == -fin["z0_inv"] * sum(pow(v, i, R) * fin["z"][i] * om.evaluate(sm.lagrange(s["pts"], s["ebar"]), u) for i, s in enumerate(o["prep"]["sets"])) % R


def test_with_one_evaluation_changed_the_partial_form_stands_and_the_report_names_the_set():
    n, wrong = 64, (2, 0, 1)
    p, pts, columns, evals, y, v, u = small_stage(n, sc.SETS, wrong=wrong)
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    assert o["report"]["bad_sets"] == 1 and o["report"]["first_bad_set"] == 2 and o["report"]["last_remainder"] != 0
    of_set = [pts[q] for q in p.sets[2][0]]
    # the changed value moves R_2 by a multiple of one Lagrange basis polynomial: the remainder at its point alone is not 0
    assert [bool(r) for r in o["rems"][2]] == [False, True, False] and not any(any(r) for i, r in enumerate(o["rems"]) if i != 2)
    # both forms are then the polynomial quotient of N_2 by Z_2, the remainder (the interpolant of N_2 at the points) dropped
    q = sm.partial_quotient(o["numer"][2], of_set)[0]
    assert sm.halo2_quotient(columns[2], evals[2], of_set, y) == q and times(q, vanishing(of_set), n) != o["numer"][2]
    _p, _pts, _columns, own = small_stage(n, sc.SETS)[:4]
    good = sm.opening(p, columns, own, pts, y, v, lambda _h: u)
    assert good["numer"][2] != o["numer"][2] and good["numer"][3] == o["numer"][3]


def test_two_equal_points_in_a_set_are_counted_and_weigh_nothing():
    w, zero = sm.weights([5, 7, 5])
    assert zero == 2 and w[0] == w[2] == 0 and w[1] == sm.inv((7 - 5) * (7 - 5) % R)


def test_multiopen_plan_groups_the_queries_by_first_appearance(pkg):
    plan = pkg.api.multiopen_plan([("a", 0), ("z", 1), ("z", 0), ("b", 0), ("p", -1), ("p", 0), ("p", 1), ("c", 0), ("q", 1), ("q", 0)])
    assert plan.rotations == [0, 1, -1]
    assert plan.sets == [((0,), ["a", "b", "c"]), ((0, 1), ["z", "q"]), ((0, 1, 2), ["p"])]
    assert (plan.set_points, plan.set_cols, plan.point_index) == ([1, 2, 3], [3, 2, 1], [0, 0, 1, 0, 1, 2])
    assert plan.eval_order() == [("a", 0), ("b", 0), ("c", 0), ("z", 0), ("z", 1), ("q", 0), ("q", 1), ("p", 0), ("p", 1), ("p", -1)]
    assert pkg.api.multiopen_plan([]).sets == [] and pkg.api.multiopen_plan([(1, 5), (1, 5)]).eval_order() == [(1, 5)]
    mine = sc.plan()
    again = pkg.api.multiopen_plan([(c, q) for idx, cols in mine.sets for c in cols for q in idx])
    assert sorted(again.rotations) == list(range(8)) and again.set_cols == mine.set_cols and again.set_points == mine.set_points


def test_the_constants_and_the_sizes(drivers, pkg):
    api, lib = pkg.api, pkg.api.load_shplonk_library()
    *cells, report_bytes = [int(v) for v in drivers("constants")[0].split()]
    assert len(cells) == len(api.SHPLONK_TABLES) == 13 and cells[0] == 0 and cells == sorted(cells) and report_bytes == 64 == int(lib.aesw_shplonk_report_bytes())
    assert [int(lib.aesw_shplonk_scalars_offset(t, 0)) for t in range(13)] == [32 * c for c in cells]
    none = (1 << 64) - 1
    assert int(lib.aesw_shplonk_scalars_offset(13, 0)) == none and int(lib.aesw_shplonk_scalars_offset(7, 1)) == none and int(lib.aesw_shplonk_scalars_offset(2, 16)) == none
    assert int(lib.aesw_shplonk_scalars_offset(9, 16)) == 32 * (cells[9] + 16) and int(lib.aesw_shplonk_scalars_offset(3, 2)) == 32 * (cells[3] + 16)
    open_lib = api.load_open_library()
    for n_sets, max_cols, k in ((1, 1, 10), (4, 5, 11), (16, 65535, 28), (3, 7, 19)):
        scalars, ws = [int(v) for v in drivers("sizes", n_sets, max_cols, k)[0].split()]
        assert scalars == 32 * (cells[12] + max_cols) == int(lib.aesw_shplonk_scalars_bytes(n_sets, max_cols)) and scalars % 16 == 0
        assert ws == int(lib.aesw_shplonk_workspace_bytes(k)) == int(open_lib.aesw_open_workspace_bytes(k, 1, 8)) and ws % 16 == 0
    for n_sets, max_cols, k in ((0, 1, 9), (17, 1, 29), (1, 0, 9), (1, 65536, 29)):
        assert [int(v) for v in drivers("sizes", n_sets, max_cols, k)[0].split()] == [0, 0]
        assert int(lib.aesw_shplonk_scalars_bytes(n_sets, max_cols)) == 0 and int(lib.aesw_shplonk_workspace_bytes(k)) == 0


def test_the_header_refuses_a_plan_that_is_none(drivers):
    d = drivers.dir
    for text, word in (("8 1\n1 1 0\n", None), ("0 1\n1 1 0\n", "n_points"), ("17 1\n1 1 0\n", "n_points"), ("8 0\n", "n_sets"), ("8 17\n" + "1 1 0\n" * 17, "n_sets"),
                       ("8 1\n0 1\n", "set_points"), ("8 1\n9 1 0 1 2 3 4 5 6 7 8\n", "set_points"), ("8 1\n1 0 0\n", "set_cols"), ("8 1\n1 65536 0\n", "set_cols"),
                       ("8 1\n1 1 8\n", "below n_points"), ("8 2\n1 1 0\n2 1 3 3\n", "increasing"), ("8 1\n2 1 4 2\n", "increasing")):
        (d / "plan.txt").write_text(text)
        out = drivers("plan", d / "plan.txt")[0]
        assert out.startswith("0" if word is None else "1") and (word is None or word in out), (text, out)


def write_stage(d, stage):
    p, pts, columns, evals, y, v, u = stage
    (d / "plan.txt").write_text(p.text())
    cells = pts + [y, v, u] + sc.flat_evals(evals) + [c for of_set in columns for column in of_set for c in column]
    nm.to_cells(cells).tofile(d / "cells.bin")


def held(raw, k, p, o, cells_at):
    """the driver's (or the device's) output `raw` against the model `o`, table by table"""
    n = 1 << k
    block_cells = cells_at[12] + max(p.set_cols)
    take = lambda first, count: nm.from_cells(raw[32 * first:32 * (first + count)].reshape(-1, 32))  # noqa: E731
    table = dict(zip(("plan", "v_pow", "ebar", "w", "vw", "neg_r", "z", "z_t", "z0_inv", "l_coef", "l_const", "l_low", "y_pow"), cells_at))
    prep, fin, S = o["prep"], o["fin"], len(p.sets)
    words = struct.unpack("<256I", raw[:1024].tobytes())
    assert words[:3] == (len(p.rotations), S, max(p.set_cols)) and list(words[16:16 + S]) == p.set_points and list(words[32:32 + S]) == p.set_cols
    assert [list(words[128 + 8 * i:128 + 8 * i + t]) for i, t in enumerate(p.set_points)] == [list(idx) for idx, _cols in p.sets]
    assert take(table["y_pow"], max(p.set_cols)) == prep["y_pow"] and take(table["v_pow"], 16) == prep["v_pow"] + [0] * (16 - S)
    pad = lambda rows: [x for row in rows for x in list(row) + [0] * (8 - len(row))] + [0] * (8 * (16 - len(rows)))  # noqa: E731
    for name in ("ebar", "w", "vw", "neg_r"):
        assert take(table[name], 128) == pad([s[name] for s in prep["sets"]]), name
    assert take(table["z"], 16) == fin["z"] + [0] * (16 - S) and take(table["z_t"], 1) == [fin["z_t"]] and take(table["z0_inv"], 1) == [fin["z0_inv"]]
    assert take(table["l_coef"], 17) == fin["l_coef"] + [0] * (16 - S) and take(table["l_const"], 1) == [fin["l_const"]] and take(table["l_low"], 8) == fin["l_low"]
    at = block_cells
    for i in range(S):
        assert take(at, n) == o["numer"][i], i
        assert take(at + n, 8) == o["rems"][i] + [0] * (8 - len(o["rems"][i])), i
        at += n + 8
    assert take(at, n) == o["h"] and take(at + n, n) == o["line"] and take(at + 2 * n, n) == o["w"]
    report = struct.unpack("<8Q", raw[32 * (at + 3 * n):].tobytes())
    rep = o["report"]
    assert report[:4] == (rep["bad_sets"], (1 << 64) - 1 if rep["first_bad_set"] is None else rep["first_bad_set"], rep["zero_differences"], rep["z0_zero"])
    assert nm.from_cells(np.frombuffer(struct.pack("<4Q", *report[4:]), np.uint8).reshape(1, 32)) == [rep["last_remainder"]]


@pytest.mark.parametrize("build", sorted(FLAGS))
@pytest.mark.parametrize("k", sc.KS + ("full",))
def test_the_cpu_run_of_the_kernels_is_the_model(drivers, build, k):
    d = drivers.dir
    cells_at = [int(v) for v in drivers("constants")[0].split()][:13]
    stage, k = (sc.full_stage(), sc.FULL_K) if k == "full" else (sc.stage(k), k)  # full: sc.FULL_SETS, 16 sets over 16 points, up to 257 columns
    p, pts, columns, evals, y, v, u = stage
    write_stage(d, stage)
    drivers("stage", k, d / "plan.txt", d / "cells.bin", d / "out.bin", build=build)
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    assert o["report"]["bad_sets"] == 0 and o["report"]["last_remainder"] == 0
    held(np.fromfile(d / "out.bin", np.uint8), k, p, o, cells_at)


def test_a_wrong_evaluation_and_two_equal_points_on_the_cpu(drivers):
    d, k = drivers.dir, 10
    cells_at = [int(v) for v in drivers("constants")[0].split()][:13]
    p, pts, columns, evals, y, v, u = sc.stage(k, wrong=(3, 4, 7))
    write_stage(d, (p, pts, columns, evals, y, v, u))
    drivers("stage", k, d / "plan.txt", d / "cells.bin", d / "out.bin")
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    assert o["report"]["bad_sets"] == 1 and o["report"]["first_bad_set"] == 3 and o["report"]["last_remainder"] != 0
    held(np.fromfile(d / "out.bin", np.uint8), k, p, o, cells_at)
    # two equal points: super-set points 5 and 6 hold one value; set 3 has both
    pts = list(pts)
    pts[6] = pts[5]
    p, _pts, columns, _evals, y, v, u = sc.stage(k)
    evals = [[[om.evaluate(column, pts[q]) for q in idx] for column in columns[i]] for i, (idx, _cols) in enumerate(p.sets)]
    write_stage(d, (p, pts, columns, evals, y, v, u))
    drivers("stage", k, d / "plan.txt", d / "cells.bin", d / "out.bin")
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    assert o["report"]["zero_differences"] == 2
    held(np.fromfile(d / "out.bin", np.uint8), k, p, o, cells_at)


def test_the_full_plan_is_what_it_says():
    p, pts, _columns, _evals, _y, _v, _u = sc.full_stage()
    assert len(set(pts)) == len(pts) == 16 == len(p.sets) == len(p.rotations) and pts[:4] == [0, 1, nm.omega(sc.FULL_K), R - 1]
    assert sorted(set(p.set_points)) == list(range(1, 9)) and {q for idx, _cols in p.sets for q in idx} == set(range(16))
    assert p.sets[15][0] == tuple(range(8, 16)) and p.set_points[0] == 2 and all(list(idx) == sorted(set(idx)) for idx, _cols in p.sets)
    assert sorted((t, m) for t, m in zip(p.set_points, p.set_cols) if m != 1) == [(1, sc.WIDE_COLS), (8, 3)] and p.set_cols[sc.WIDE_SET] == sc.WIDE_COLS == 257


def opened(stage):
    p, pts, columns, evals, y, v, u = stage
    return sm.opening(p, columns, evals, pts, y, v, lambda _h: u)


def test_what_u_on_a_point_and_challenges_of_0_and_1_do_to_the_model():
    on_a_point = sc.u_on_a_point()
    p, pts, _columns, _evals, _y, _v, u = on_a_point["u_outside_set_0"]
    o = opened(on_a_point["u_outside_set_0"])
    fin = o["fin"]
    assert pts.index(u) not in p.sets[0][0] and fin["z"][0] == 0 and fin["z_t"] == 0 and o["report"]["z0_zero"] == 1
    # fr_inv(0) = 0: every coefficient of L' is zero, and L' with them
    assert fin["z0_inv"] == 0 and fin["l_coef"] == [0] * 17 and fin["l_const"] == 0 and fin["l_low"] == [0] * 8 and not any(o["line"]) and any(fin["z"])
    p, pts, _columns, _evals, _y, _v, u = on_a_point["u_inside_set_0"]
    o = opened(on_a_point["u_inside_set_0"])
    fin = o["fin"]
    assert pts.index(u) in p.sets[0][0] and fin["z_t"] == 0 and fin["z"][0] != 0 and o["report"]["z0_zero"] == 0 and fin["l_coef"][16] == 0 and any(fin["l_coef"][:16])
    assert any(o["line"]) and om.evaluate(o["line"], u) == 0 and o["report"]["last_remainder"] == 0
    stages = sc.degenerate_stages()
    for name in ("y=0", "y=0,u=0"):
        _p, _pts, columns, _evals, y, _v, _u = stages[name]
        o = opened(stages[name])
        assert y == 0 and o["prep"]["y_pow"] == [1, 0, 0, 0, 0]  # 0^0 is 1
        for i, s in enumerate(o["prep"]["sets"]):  # N_i is the set's first column plus the low cells
            assert o["numer"][i] == [(c + s["neg_r"][d]) % R if d < len(s["neg_r"]) else c for d, c in enumerate(columns[i][0])], i
        assert o["report"]["bad_sets"] == 0 and o["report"]["last_remainder"] == 0
    for name in ("v=0", "v=0,u=0"):
        o = opened(stages[name])
        q0, _rems = sm.partial_quotient(o["numer"][0], o["prep"]["sets"][0]["pts"])
        assert stages[name][5] == 0 and o["prep"]["v_pow"] == [1, 0, 0, 0] and o["h"] == q0 and any(q0)  # h is Q_0 alone, scaled by v^0 = 1
        assert all(not any(s["vw"]) for s in o["prep"]["sets"][1:]) and o["report"]["last_remainder"] == 0
    for name in ("y=v=1", "y=v=1,u=0"):
        o = opened(stages[name])
        assert o["prep"]["y_pow"] == [1] * 5 and o["prep"]["v_pow"] == [1] * 4 and o["report"]["last_remainder"] == 0
    for name, stage in stages.items():  # u = 0 is super-set point 0, which set 0 of sc.SETS does not hold: z_0 = 0 and L' is zero
        o = opened(stage)
        at_zero = name.endswith("u=0")
        assert (stage[6] == 0) == at_zero and o["report"]["z0_zero"] == int(at_zero) and any(o["line"]) != at_zero and (o["fin"]["l_coef"] == [0] * 5) == at_zero, name


@pytest.mark.parametrize("name", sorted(sc.u_on_a_point()) + sorted(sc.degenerate_stages()))
def test_the_cpu_run_with_u_on_a_point_and_with_challenges_of_0_and_1_is_the_model(drivers, name):
    d = drivers.dir
    cells_at = [int(v) for v in drivers("constants")[0].split()][:13]
    stage = {**sc.u_on_a_point(), **sc.degenerate_stages()}[name]
    k = sc.FULL_K
    write_stage(d, stage)
    drivers("stage", k, d / "plan.txt", d / "cells.bin", d / "out.bin")
    held(np.fromfile(d / "out.bin", np.uint8), k, stage[0], opened(stage), cells_at)


@pytest.mark.parametrize("build,t", (("plain", 2), ("plain", 3), ("sanitized", 2)))
def test_the_second_turn_of_the_carry_is_the_serial_recurrence(drivers, build, t):
    assert drivers("check", sc.REACH_K, 0x7368, t, build=build) == ["0"]
    if build == "plain":
        assert drivers("check", 11, 0x7369, 8) == ["0"] and drivers("check", 10, 0x736a, 1) == ["0"]
