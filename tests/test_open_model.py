"""The specification of libaesw_open.so without a GPU.

tests/open_model.py -- evaluate, fold and divide, each the serial definition in Python integers -- is held against itself: divide's
q(X) (X - z) + rem is the column again, coefficient by coefficient, rem is evaluate, and evaluate is ntt_model's Horner.
csrc/aesw_open.h -- the bounds, the chunks and the turns, the index of every power z^(2^s), the workspace, the recurrence and the
pieces the passes join -- is compiled alone with g++ into tests/open_driver.cpp, a program of its own that executes the powers,
chunk, carry and scan passes of open/aesw_open.hip on the CPU through those functions, lane by lane, and is held against the model
cell for cell at k = 10 (one chunk) and k = 11 (a carry across two chunks), once plain and once under
-fsanitize=address,undefined.  The second turn of the carry (k = 19, 512 chunks) and k = 20 are above what a test should spend
in Python: there the driver holds the passes against the header's own serial recurrence, which the model pins at k = 10 and 11."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ntt_model as nm
import open_cases as oc
import open_model as om

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("open_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("open_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "open_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def cells_file(path, values):
    nm.to_cells(values).tofile(path)
    return path


def values_of(path):
    return nm.from_cells(np.fromfile(path, np.uint8).reshape(-1, 32))


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_open.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text and '#include "aesw_fr.h"' in text
    assert text.count("#include \"aesw") == 1  # the field alone


@pytest.mark.parametrize("n", (1, 2, 5, 64))
def test_the_model_divides_back_to_the_column_and_its_remainder_is_the_value(n):
    coeff = nm.seeded_values(n, 0x6f70 + n)
    for z in oc.points(6, 0x7a + n):
        q, rem = om.divide(coeff, z)
        assert q[-1] == 0 and rem == om.evaluate(coeff, z) == nm.evaluate(coeff, z)
        assert om.times_linear(q, z, rem) == coeff
    assert om.divide(coeff, 0) == (coeff[1:] + [0], coeff[0])


def test_the_model_folds_in_the_order_of_the_header():
    a, b, c, acc = (nm.seeded_values(4, s) for s in (1, 2, 3, 4))
    v = nm.seeded_values(1, 5)[0]
    assert om.fold([a, b, c], v) == [(x * v * v + y * v + z) % nm.R for x, y, z in zip(a, b, c)]
    assert om.fold([c], v, om.fold([a, b], v, acc)) == om.fold([a, b, c], v, acc) == [(w * v ** 3 + x * v * v + y * v + z) % nm.R for w, x, y, z in zip(acc, a, b, c)]
    # the evaluation of a fold is the fold of the evaluations
    z = nm.seeded_values(1, 6)[0]
    assert om.evaluate(om.fold([a, b], v), z) == (om.evaluate(a, z) * v + om.evaluate(b, z)) % nm.R


def test_the_constants_and_the_sizes(drivers, pkg):
    chunk, rows, turn, powers, p_cell, p_lane, p_wave, p_chunk, p_chunk_wave = [int(v) for v in drivers("constants")[0].split()]
    assert (chunk, rows, turn, powers) == (oc.CHUNK, 4, oc.TURN, 29) and chunk == 256 * rows
    # a power's index is the binary logarithm of the piece it skips: a cell, a lane's cells, a wave's, a chunk, a wave of chunks
    assert [1 << p for p in (p_cell, p_lane, p_wave, p_chunk, p_chunk_wave)] == [1, rows, 64 * rows, chunk, 64 * chunk]
    lib = pkg.api.load_open_library()
    for k, n_cols, n_points in ((10, 1, 1), (11, 3, 3), (18, 2, 16), (19, 1, 1), (20, 8, 4), (28, 65535, 16)):
        ws, chunks, turns, *firsts = [int(v) for v in drivers("sizes", k, n_cols, n_points)[0].split()]
        assert chunks == (1 << k) // chunk and turns == -(-chunks // turn)
        assert ws == 32 * (powers * n_points + n_cols * n_points * chunks) == int(lib.aesw_open_workspace_bytes(k, n_cols, n_points)) and ws % 16 == 0
        assert firsts == [(turns - 1 - t) * turn for t in range(min(turns, 4))]  # from the last chunk down
    assert int(drivers("sizes", oc.REACH_K, 1, 1)[0].split()[2]) == 2 and int(drivers("sizes", oc.REACH_K - 1, 1, 1)[0].split()[2]) == 1
    for k, n_cols, n_points in ((9, 1, 1), (29, 1, 1), (10, 0, 1), (10, 65536, 1), (10, 1, 0), (10, 1, 17), (1 << 31, 1, 1)):
        assert int(lib.aesw_open_workspace_bytes(k, n_cols, n_points)) == 0 and int(drivers("sizes", k, n_cols, n_points)[0].split()[0]) == 0


@pytest.mark.parametrize("build", sorted(FLAGS))
@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "k%d-c%d-p%d" % s)
def test_the_cpu_run_of_the_passes_is_the_model(drivers, build, shape):
    k, n_cols, n_points = shape
    d = drivers.dir
    columns = [nm.seeded_values(1 << k, 0x6f64 + 8 * k + c) for c in range(n_cols)]
    columns[-1] = [0] * ((1 << k) - 1) + [columns[-1][-1]] if n_cols > 1 else columns[-1]  # only the top coefficient set
    coeff = cells_file(d / "coeff.bin", [v for column in columns for v in column])
    pts = oc.points(k, 0x7074 + k)
    for first in range(0, len(pts), n_points):
        some = (pts[first:first + n_points] + pts)[:n_points]
        drivers("evaluate", k, n_cols, n_points, coeff, cells_file(d / "points.bin", some), d / "evals.bin", build=build)
        assert values_of(d / "evals.bin") == [om.evaluate(column, z) for column in columns for z in some], (shape, first)
    for z in pts:
        point = cells_file(d / "point.bin", [z])
        expected = [om.divide(column, z) for column in columns]
        drivers("divide", k, n_cols, coeff, point, d / "quot.bin", d / "rem.bin", build=build)
        assert values_of(d / "quot.bin") == [v for q, _rem in expected for v in q] and values_of(d / "rem.bin") == [rem for _q, rem in expected], (shape, z)
        if build == "plain":
            drivers("serial", k, cells_file(d / "one.bin", columns[0]), point, d / "serial.bin", d / "serial_rem.bin")
            assert values_of(d / "serial.bin") == expected[0][0] and values_of(d / "serial_rem.bin") == [expected[0][1]]
    # in place, at the last point
    same = cells_file(d / "same.bin", [v for column in columns for v in column])
    drivers("divide", k, n_cols, same, point, same, d / "rem.bin", build=build)
    assert values_of(same) == [v for q, _rem in expected for v in q]
    # the fold: no accumulator, and one
    v = nm.seeded_values(1, 0x76 + k)[0]
    acc = nm.seeded_values(1 << k, 0x6163 + k)
    drivers("fold", k, n_cols, coeff, cells_file(d / "v.bin", [v]), "-", d / "folded.bin", build=build)
    assert values_of(d / "folded.bin") == om.fold(columns, v)
    drivers("fold", k, n_cols, coeff, d / "v.bin", cells_file(d / "acc.bin", acc), d / "folded.bin", build=build)
    assert values_of(d / "folded.bin") == om.fold(columns, v, acc)


@pytest.mark.parametrize("k,build", ((oc.REACH_K, "plain"), (oc.REACH_K + 1, "plain"), (oc.REACH_K, "sanitized")))
def test_the_second_turn_of_the_carry_is_the_serial_recurrence(drivers, k, build):
    seeded = nm.seeded_values(1, 0x7475 + k)[0]
    for z in ((0, 1, seeded) if build == "plain" else (seeded,)):
        assert drivers("check", k, k, "%064x" % (z * nm.MONT % nm.R), build=build) == ["0"], (k, z)
