"""The specification of the quotient without a GPU (the fold has no kernel yet; libaesw_quot.so holds sigma as
cells, whose rule is held here too).

tests/quot_model.py is held against the definition at k = 3, ext_k = 5, n_sets = 1: every column a random Lagrange column turned
into coefficients by ntt_model, its polynomial evaluated by Horner at x_j and at x_j * omega^r for a rotation, l0, l_last and
l_active the polynomials of their unit columns, delta^c * x_j from the point itself; the constraints written out here once more
and folded.  csrc/aesw_quot.h -- the bounds, the rotation, the vanishing index, the products per row, the tables, the label of a
mapping entry and the fold -- is compiled alone with g++ into tests/quot_driver.cpp, which runs the fold of every row at k = 10,
ext_k = 12, n_sets = 2 through the header's functions; it is held against the model on every row, once plain and once under
-fsanitize=address,undefined."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ntt_model as nm
import quot_cases as qc
import quot_model as qm
import sigma_model as sm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
R = nm.R


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("quot_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("quot_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "quot_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def plain(hex_cell):
    return int(hex_cell, 16) * nm.MONT_INV % R


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_quot.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text


@pytest.mark.parametrize("chunk_len,n_rows,zeta_sel", ((3, 5, 1), (2, 4, 0)))
def test_the_model_is_the_definition(chunk_len, n_rows, zeta_sel):
    k, ext_k, n_sets = 3, 5, 1
    n, m = 1 << k, 1 << (ext_k - k)
    counts = qm.group_columns(n_sets, chunk_len)
    lagrange = {g: [nm.seeded_values(n, 0x71 + 97 * i + c) for c in range(count)] for i, (g, count) in enumerate(counts.items())}
    lagrange["l"] = qm.unit_columns(k, n_rows)
    coeff = {g: [nm.lagrange_to_coeff(col, k) for col in cols] for g, cols in lagrange.items()}
    extended = {g: [nm.coeff_to_extended(col, k, ext_k, zeta_sel) for col in cols] for g, cols in coeff.items()}
    theta, beta, gamma, y = nm.seeded_values(4, 0x7175)
    w, w_ext, zeta = nm.omega(k), nm.omega(ext_k), nm.ZETAS[zeta_sel]
    sets = sm.sets_of(5, chunk_len)
    assert len(sets) == counts["zperm"] and pow(w_ext, m, R) == w
    got = qm.quotient(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, extended, theta, beta, gamma, y)
    for j in range(1 << ext_k):
        x = zeta * pow(w_ext, j, R) % R

        def p(g, c, r=0):
            return nm.evaluate(coeff[g][c], x * pow(w, r % n, R) % R)
        l0, l_last, l_active = p("l", 0), p("l", 1), p("l", 2)
        # the unit columns' polynomials: l_blind covers the rows above U
        assert l_active == (1 - l_last - sum(nm.evaluate(nm.lagrange_to_coeff([int(i == b) for i in range(n)], k), x) for b in range(n_rows + 1, n))) % R
        words, rcon, q_rcon = p("advice", 3), p("rcon", 0), p("rcon", 1)
        v = [p("advice", 0), p("advice", 1), p("advice", 2), words, rcon]  # x0 y0 z0 words rcon
        cons = [q_rcon * (words - rcon), l0 * (1 - p("zperm", 0)), l_last * (p("zperm", len(sets) - 1) ** 2 - p("zperm", len(sets) - 1))]
        cons += [l0 * (p("zperm", s) - p("zperm", s - 1, n_rows)) for s in range(1, len(sets))]
        for s, (first, end) in enumerate(sets):
            left, right = p("zperm", s, 1), p("zperm", s)
            for c in range(first, end):
                left *= v[c] + beta * p("sigma", c) + gamma
                right *= v[c] + beta * pow(sm.DELTA, c, R) * x + gamma
            cons.append(l_active * (left - right))
        for t, a in ((1, 2), (2, 4), (3, 3), (4, 3), (5, 3)):
            q, i = p("selectors", t - 1), t - 1
            inp = tab = 0
            for e in range(a):
                inp = inp * theta + q * (t, v[0], v[1], v[2])[e]
                tab = tab * theta + p("table", e)
            z, ap, sp = p("zlookup", i), p("a", i), p("s", i)
            cons += [l0 * (1 - z), l_last * (z * z - z), l_active * (p("zlookup", i, 1) * (ap + beta) * (sp + gamma) - z * (inp + beta) * (tab + gamma)),
                     l0 * (ap - sp), l_active * (ap - sp) * (ap - p("a", i, -1))]
        acc = 0
        for c in cons:
            acc = (acc * y + c) % R
        assert len(cons) == 3 + (len(sets) - 1) + len(sets) + 25
        assert got[j] == acc * pow(pow(x, n, R) - 1, -1, R) % R, j


def test_rotations_the_vanishing_index_the_counts_and_the_bounds(drivers):
    for k, ext_k, j, r in ((10, 12, 0, 1), (10, 12, 4095, 1), (10, 12, 0, -1), (10, 12, 3, -1), (10, 12, 5, 1018), (10, 13, 8191, 1015), (17, 19, 12345, (1 << 17) - 6),
                           (20, 28, (1 << 28) - 1, (1 << 20) - 1), (26, 28, 0, -1)):
        assert int(drivers("rot", k, ext_k, j, r)[0]) == qm.rot(k, ext_k, j, r) == (j + r * (1 << (ext_k - k))) % (1 << ext_k)
        assert int(drivers("vanish", k, ext_k, j)[0]) == j % (1 << (ext_k - k))
    for n_sets, chunk_len in ((1, 3), (2, 3), (1, 2), (4, 3), (4, 8), (1024, 1)):
        assert int(drivers("products", n_sets, chunk_len)[0]) == qm.products_per_row(n_sets, chunk_len)
        counts = [int(v) for v in drivers("columns", n_sets, chunk_len)[0].split()]
        assert counts[:-1] == list(qm.group_columns(n_sets, chunk_len).values()) and counts[-1] == sum(counts[:-1])
    assert qm.products_per_row(4, 3) == 436 and sum(qm.group_columns(4, 3).values()) == 121
    ok = lambda *shape: int(drivers("ok", *shape)[0])  # noqa: E731
    assert ok(10, 12, 1, 1, 3, 1018) and ok(10, 12, 0, 1024, 1, 1) and ok(26, 28, 1, 4, 3, (1 << 26) - 1) and ok(10, 14, 1, 1, 8, 1023)
    for bad in ((9, 12, 1, 1, 3, 100), (10, 11, 1, 1, 3, 100), (27, 29, 1, 1, 3, 100), (10, 12, 2, 1, 3, 100), (10, 12, 1, 0, 3, 100), (10, 12, 1, 1025, 3, 100),
                (10, 12, 1, 1, 0, 100), (10, 12, 1, 1, 4, 100), (10, 13, 1, 1, 8, 100), (10, 14, 1, 1, 9, 100), (10, 12, 1, 1, 3, 0), (10, 12, 1, 1, 3, 1024)):
        assert not ok(*bad), bad


def test_the_tables_and_their_sizes(drivers):
    for k, ext_k in ((10, 12), (10, 13), (13, 15), (20, 22), (25, 28), (10, 28)):
        size, vanish_at, low_at, high_at, cells = [int(v) for v in drivers("sizes", k, ext_k)[0].split()]
        m = 1 << (ext_k - k)
        assert (vanish_at, low_at, high_at, cells) == (0, m, m + (1 << min(ext_k, 14)), m + (1 << min(ext_k, 14)) + (1 << max(ext_k - 14, 0)))
        assert size == 32 * cells
    for k, ext_k in ((9, 12), (10, 11), (27, 29), (12, 10)):
        assert int(drivers("sizes", k, ext_k)[0].split()[0]) == 0
    for k, ext_k, sel in ((10, 12, 1), (11, 13, 0), (13, 16, 1)):
        exp = qm.tables(k, ext_k, sel)
        m = 1 << (ext_k - k)
        at = sorted(set(range(m)) | {m, m + 1, m + (1 << min(ext_k, 14)) - 1, len(exp) - 1, len(exp) - (1 << max(ext_k - 14, 0))})
        assert [plain(v) for v in drivers("table", k, ext_k, sel, *at)] == [exp[i] for i in at]
        x = [qm.point(ext_k, sel, j) for j in range(m)]
        assert all((pow(xj, 1 << k, R) - 1) * exp[j] % R == 1 for j, xj in enumerate(x))


def test_the_label_of_a_mapping_entry(drivers):
    for k, n_cols, c, i, entry in ((10, 5, 2, 7, 3 * 1024 + 1000), (10, 5, 2, 7, 5 * 1024), (15, 5, 4, 20000, 4 * 32768 + 32767), (15, 5, 0, 3, 0xffffffff),
                                   (15, 5, 1, 16384, 16384)):
        image = entry if entry < n_cols << k else (c << k) + i
        lines = drivers("label", k, n_cols, c, i, entry)
        assert int(lines[0]) == image
        w_pows = {image & ((1 << k) - 1): pow(sm.omega(k), image & ((1 << k) - 1), R)}
        assert plain(lines[1]) == sm.label(k, w_pows, [pow(sm.DELTA, cc, R) for cc in range(n_cols)], image)


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_cpu_run_of_the_fold_is_the_model_on_every_row(drivers, build):
    k, ext_k, sel, n_sets, chunk_len, blind = qc.DRIVER
    n_rows = (1 << k) - blind
    cells, values = qm.seeded_columns(ext_k, n_sets, chunk_len, 0x64727672)
    challenges = nm.seeded_values(4, 0x6368)
    src, dst = drivers.dir / "in.bin", drivers.dir / "out.bin"
    np.concatenate([qm.cells_of(cells), nm.to_cells(challenges)]).tofile(src)
    drivers("run", k, ext_k, sel, n_sets, chunk_len, n_rows, src, dst, build=build)
    got = np.fromfile(dst, np.uint8).reshape(-1, 32)
    exp = qm.quotient(k, ext_k, sel, n_sets, chunk_len, n_rows, values, *challenges)
    assert got.shape == (1 << ext_k, 32) and np.array_equal(got, nm.to_cells(exp))
