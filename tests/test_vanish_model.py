"""The segments of the quotient without a GPU.

tests/vanish_model.py is held against quot_model: its segments one behind the other are quot_model.constraints, their folds one
into the other quot_model.fold, and every segment from an arbitrary acc_in is acc_in * y^len + the segment from 0.
csrc/aesw_vanish.h -- the segment list, the lengths, the products per row, the scalars block and its layout, the four segments --
is compiled alone with g++ into tests/vanish_driver.cpp, which at quot_cases.DRIVER's shape holds on every row that the segments in
their order are quot_numerator and that each is linear in acc_in, and whose quotient after the division is held against
quot_model.quotient; once plain and once under -fsanitize=address,undefined."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ntt_model as nm
import quot_cases as qc
import quot_model as qm
import vanish_model as vm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
R = nm.R
SHAPES = ((1, 3), (2, 3), (2, 2), (1, 2), (4, 3), (4, 8), (3, 1))  # (n_sets, chunk_len)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("vanish_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("vanish_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "vanish_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.returncode, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_vanish.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text and '#include "aesw_quot.h"' in text


@pytest.mark.parametrize("n_sets,chunk_len", ((1, 3), (2, 2), (2, 3)))
def test_the_segments_one_behind_the_other_are_the_constraints_and_their_folds_the_fold(n_sets, chunk_len):
    k, ext_k, zeta_sel, n_rows = 3, 5, 1, 5
    _cells, values = qm.seeded_columns(ext_k, n_sets, chunk_len, 0x766d + n_sets)
    theta, beta, gamma, y = nm.seeded_values(4, 0x7663 + chunk_len)
    sc = vm.scalars(n_sets, chunk_len, theta, beta, gamma, y)
    segs = vm.segments(n_sets, chunk_len)
    assert [kind for kind, _s in segs] == ["head"] + ["perm"] * qm.perm_sets(n_sets, chunk_len) + ["lookup"] * n_sets + ["divide"]
    seeded = nm.seeded_values(1 << ext_k, 0x7661)
    for j in range(1 << ext_k):
        x = qm.point(ext_k, zeta_sel, j)
        at = lambda g, c, r: values[g][c][qm.rot(k, ext_k, j, r)]  # noqa: E731
        want = qm.constraints(k, ext_k, n_sets, chunk_len, n_rows, x, at, theta, beta, gamma)
        got = [v for kind, s in segs for v in vm.segment_values(kind, s, n_sets, chunk_len, n_rows, x, at, sc)]
        assert got == want, j
        cell = lambda g, c, r: values[g][c][r]  # noqa: E731
        acc = 0
        for kind, s in segs[:-1]:
            args = (kind, s, k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, j, cell, sc)
            length = vm.segment_len(kind, n_sets, chunk_len)
            assert length == len(vm.segment_values(kind, s, n_sets, chunk_len, n_rows, x, at, sc))
            assert vm.run_segment(*args, acc_in=seeded[j]) == (seeded[j] * pow(y, length, R) + vm.run_segment(*args)) % R
            assert sc["y_pow"][vm.KINDS.index(kind)] == pow(y, length, R)
            acc = vm.run_segment(*args, acc_in=acc)
        assert acc == qm.fold(want, y)
    rows = [0, 1, 7, 31]
    assert vm.quotient(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, values, theta, beta, gamma, y, rows) == \
        qm.quotient(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, values, theta, beta, gamma, y, rows)


def test_the_segment_list_the_lengths_and_the_products(drivers):
    for n_sets, chunk_len in SHAPES + ((1024, 1),):
        lines = [[int(v) for v in line.split()] for line in drivers("segments", n_sets, chunk_len)]
        segs = vm.segments(n_sets, chunk_len)
        assert [(vm.KINDS[kind], s) for kind, s, _len, _p, _o in lines[:-1]] == segs
        assert [length for _k, _s, length, _p, _o in lines[:-1]] == [vm.segment_len(kind, n_sets, chunk_len) for kind, _s in segs]
        assert [p for _k, _s, _len, p, _o in lines[:-1]] == [vm.segment_products(kind, s, n_sets, chunk_len) for kind, s in segs]
        # what a call runs is its share and its overhead
        assert [p + o for _k, _s, _len, p, o in lines[:-1]] == [vm.segment_run_products(kind, s, n_sets, chunk_len) for kind, s in segs]
        ours, whole, overhead = lines[-1]
        assert sum(length for _k, _s, length, _p, _o in lines[:-1]) == 1 + 2 + 2 * qm.perm_sets(n_sets, chunk_len) - 1 + 25 * n_sets  # the gate, the permutation, the lookups
        assert ours == whole == qm.products_per_row(n_sets, chunk_len) == vm.products_per_row(n_sets, chunk_len)  # the shares sum to the fold's own count
        assert overhead == sum(o for *_front, o in lines[:-1]) == qm.perm_sets(n_sets, chunk_len) + 3 * n_sets - 7
    assert vm.products_per_row(4, 3) == 436 and vm.segment_products("lookup", 1, 4, 3) == 87 and vm.segment_run_products("lookup", 0, 4, 3) == 90


def test_the_pieces_of_the_quotient_are_views_of_its_coefficients(pkg):
    api = pkg.api
    h = np.arange(32 * 32, dtype=np.uint8).reshape(32, 32)  # k = 3, ext_k = 5: four pieces of eight cells
    pieces = api.quotient_pieces(h, 3, 5)
    assert len(pieces) == 4 and all(p.shape == (8, 32) and np.shares_memory(p, h) and np.array_equal(p, h[8 * i:8 * i + 8]) for i, p in enumerate(pieces))
    assert len(api.quotient_pieces(h, 5, 5)) == 1 and [len(api.quotient_pieces(np.zeros((1 << e, 32), np.uint8), 10, e)) for e in (12, 13)] == [4, 8]
    # sum_i x^(n i) h_i(x) = h(x) over the views, in plain integers
    values = nm.seeded_values(32, 0x7069)
    x, cut = nm.seeded_values(1, 0x7078)[0], api.quotient_pieces(np.asarray(nm.to_cells(values)), 3, 5)
    assert sum(pow(x, 8 * i, R) * nm.evaluate(nm.from_cells(p), x) for i, p in enumerate(cut)) % R == nm.evaluate(values, x)
    for bad in ((h[:16], 3, 5), (h, 6, 5), (h.reshape(-1), 3, 5)):
        with pytest.raises(ValueError):
            api.quotient_pieces(*bad)


def test_the_scalars_block_and_its_layout(drivers):
    for n_sets, chunk_len in SHAPES:
        challenges = nm.seeded_values(4, 0x7673 + 8 * n_sets + chunk_len)
        src, dst = drivers.dir / "challenges.bin", drivers.dir / "scalars.bin"
        nm.to_cells(challenges).tofile(src)
        drivers("scalars", n_sets, chunk_len, src, dst)
        got = np.fromfile(dst, np.uint8).reshape(-1, 32)
        block = vm.scalars_block(n_sets, chunk_len, *challenges)
        assert int(drivers("sizes", n_sets, chunk_len)[0]) == 32 * len(block) == got.size
        assert np.array_equal(got, nm.to_cells(block))
        sc = vm.scalars(n_sets, chunk_len, *challenges)
        for t, name in enumerate(vm.TABLES):
            for index, value in enumerate(sc[name]):
                at = int(drivers("offset", t, index)[0])
                assert at == vm.offset(name, index) and block[at // 32] == value, (name, index)
    assert [int(drivers("offset", t, i)[0]) for t, i in ((0, 1), (3, 1), (4, 3), (5, 2), (6, 5), (7, 3074), (8, 3074), (9, 0))] == [-1] * 8
    assert int(drivers("offset", 8, 3073)[0]) == 32 * (14 + 2 * 3073 + 1)
    for bad in ((0, 3), (1025, 3), (1, 0), (1, 9)):
        assert int(drivers("sizes", *bad)[0]) == 0


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_cpu_run_of_the_segments_is_the_fold_on_every_row(drivers, build):
    k, ext_k, sel, n_sets, chunk_len, blind = qc.DRIVER
    n_rows = (1 << k) - blind
    cells, values = qm.seeded_columns(ext_k, n_sets, chunk_len, 0x64727672)
    challenges = nm.seeded_values(4, 0x6368)
    seeded = nm.seeded_values(1 << ext_k, 0x61636369)
    src, dst = drivers.dir / "in.bin", drivers.dir / "out.bin"
    np.concatenate([qm.cells_of(cells), nm.to_cells(challenges), nm.to_cells(seeded)]).tofile(src)
    drivers("run", k, ext_k, sel, n_sets, chunk_len, n_rows, src, dst, build=build)  # exit 6: not quot_numerator; exit 7: not linear in acc_in
    got = np.fromfile(dst, np.uint8).reshape(-1, 32)
    exp = qm.quotient(k, ext_k, sel, n_sets, chunk_len, n_rows, values, *challenges)
    assert got.shape == (1 << ext_k, 32) and np.array_equal(got, nm.to_cells(exp))
