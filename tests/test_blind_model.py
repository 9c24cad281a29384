"""The specification of libaesw_blind.so without a GPU.

csrc/aesw_blind.h -- the keyed hash of (seed, domain, column, row), the wide reduction, the fixed double-and-add of a term -- is
compiled alone with g++ into tests/blind_driver.cpp, a program of its own, once plain and once under -fsanitize=address,undefined,
and held against tests/blind_model.py (hashlib.blake2b and Python integers; the group is tests/msm_model.py's): the cells on seeds
of all zeros, all ones and random bytes, on domains and columns at and above 2^32 (the message words are 64-bit), on rows 0 and
2^28 - 1; the reduction on a digest whose two halves are both above r; the tail commitment lane by lane, as the kernel runs it,
over the special cells and the special points of tests/test_gpu_blind_commit.py.  Every comparison is exact."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import blind_cases as bc
import blind_model as bm
import msm_model as mm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
BUILDS = sorted(FLAGS)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("blind_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("blind_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "blind_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def test_the_header_is_free_of_hip_and_states_its_rule():
    text = (CSRC / "aesw_blind.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text
    assert '#include "aesw_msm.h"' in text and '#include "aesw_transcript.h"' in text and text.count("#include \"aesw") == 2
    assert bm.PERSON.decode() in text and "le64(domain) || le64(column) || le64(row)" in text and "static_assert(mont_is_canonical(blind_fixed_cell())" in text
    assert "BLIND_MAX_TAIL = 64" in text and "BLIND_MIN_K = 10, BLIND_MAX_K = 28, BLIND_MAX_COLS = 65535" in text
    person0, person1 = (int.from_bytes(bm.PERSON[i:i + 8], "little") for i in (0, 8))
    assert "BLIND_PERSON0 = %#xull" % person0 in text and "BLIND_PERSON1 = %#xull" % person1 in text
    # the cell of the static_assert is hashlib's
    limbs = bm.cell_bytes(bm.value(bytes(range(32)), 1, 2, 3))
    assert ", ".join("0x%08xu" % int.from_bytes(limbs[i:i + 4], "little") for i in range(0, 32, 4)) in text


def test_the_model_is_keyed_blake2b_and_its_cells_part():
    import hashlib
    seed = bc.SEED
    msg = (1).to_bytes(8, "little") + (2).to_bytes(8, "little") + (3).to_bytes(8, "little")
    assert bm.digest(seed, 1, 2, 3) == hashlib.blake2b(msg, key=seed, person=b"aesw-blind-cells", digest_size=64).digest()
    values = {bm.value(seed, d, c, r) for d in (0, 1) for c in (0, 1) for r in (0, 1)}
    assert len(values) == 8 and all(v < bm.R for v in values)
    assert bm.value(bc.SEEDS["zeros"], 0, 0, 0) != bm.value(bc.SEEDS["ones"], 0, 0, 0)
    assert bm.plain_of_cells(bm.tail_cells(seed, 10, 2, 1018, 5, 1)) == [v for column in bm.tail_values(seed, 10, 2, 1018, 5, 1) for v in column]


def test_the_constants_and_the_tail(drivers, pkg):
    lib = pkg.api.load_blind_library()
    max_tail, min_k, max_k, max_cols, bits = [int(v) for v in drivers("constants")[0].split()]
    assert (max_tail, min_k, max_k, max_cols, bits) == (bm.MAX_TAIL, 10, 28, 65535, 254) and int(lib.aesw_blind_max_tail()) == max_tail and bm.R.bit_length() == bits
    for k, first_row in ((10, 0), (10, 1018), (10, 1023), (10, 1024), (10, 960), (10, 959), (9, 0), (29, 0), (28, (1 << 28) - 1), (28, 1 << 28), (10, 1 << 40), (1 << 31, 0)):
        rows, ok = [int(v) for v in drivers("tail_rows", k, first_row)[0].split()]
        want = (1 << k) - first_row if 10 <= k <= 28 and first_row < 1 << k else 0
        assert rows == want == int(lib.aesw_blind_tail_rows(k, first_row)) and ok == (1 <= want <= max_tail), (k, first_row)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("seed", sorted(bc.SEEDS))
def test_the_cells_of_the_header_are_the_models(drivers, build, seed):
    s = bc.SEEDS[seed]
    # (domain, first_column, n_cols, first_row, rows): words at and above 2^32 and 2^63, rows 0 and 2^28 - 1
    for domain, first_column, n_cols, first_row, rows in ((0, 0, 1, 0, 3), (bc.DOMAIN, bc.FIRST_COLUMN, 3, 1018, 6), (1 << 32, (1 << 32) - 1, 2, 0, 2),
                                                          ((1 << 64) - 1, (1 << 63) + 9, 1, (1 << 28) - 1, 1), (bc.BIG_DOMAIN, 1 << 32, 1, (1 << 28) - 2, 2)):
        got = drivers("cells", s.hex(), domain, first_column, n_cols, first_row, rows, build=build)
        want = [bm.cell_bytes(bm.value(s, domain, first_column + j, first_row + i)).hex() for j in range(n_cols) for i in range(rows)]
        assert got == want, (seed, domain, first_column, first_row)


@pytest.mark.parametrize("build", BUILDS)
def test_the_reduction_where_both_halves_are_above_r(drivers, build):
    half = bm.R + 12345  # below 2^256, above r
    digests = [(1 << 512) - 1, half | half << 256, bm.R | bm.R << 256, (bm.R - 1) | (bm.R + 1) << 256, 0, 1 << 511]
    assert half < 1 << 256
    for d in digests:
        assert drivers("reduce", d.to_bytes(64, "little").hex(), build=build) == [bm.cell_bytes(d % bm.R).hex()], hex(d)


def commit_case(drivers, build, k, first_row, tails, commits, basis):
    """the driver's tail commitment of plain tails [n_cols][tail] over `basis` points onto `commits` points"""
    d = drivers.dir
    mm.scalar_cells([v for column in tails for v in column]).tofile(d / "tail.bin")
    mm.to_points(basis).tofile(d / "basis.bin")
    mm.to_points(commits).tofile(d / "commit.bin")
    drivers("commit", k, len(tails), first_row, d / "tail.bin", d / "basis.bin", d / "commit.bin", d / "out.bin", build=build)
    return mm.from_points(np.fromfile(d / "out.bin", np.uint8))


@pytest.mark.parametrize("build", BUILDS)
def test_the_tail_commitment_lane_by_lane_is_the_models(drivers, build):
    k, n = bc.K, 1 << bc.K
    basis = list(mm.known_basis(n))
    logs = (0x636f6d6d6974, 0, 0x31)
    for tail in bc.COMMIT_TAILS if build == "plain" else (6,):
        first_row = n - tail
        for n_cols in bc.COLS:
            tails = bc.commit_tail_values(tail, n_cols)
            commits = [mm.mul(logs[j], mm.GENERATOR) for j in range(n_cols)]  # column 1 comes in as the identity
            got = commit_case(drivers, build, k, first_row, tails, commits, basis)
            assert got == [bm.known_commit_tail(logs[j], tails[j], first_row) for j in range(n_cols)], (tail, n_cols)
            if tail <= 6:  # the model's two oracles agree: term by term, and by the logarithms
                assert got == [bm.commit_tail(commits[j], tails[j], basis[first_row:]) for j in range(n_cols)]
    # the special points: a tail that cancels the commitment, a basis point that is the identity, two rows over equal points
    tail, first_row = 6, n - 6
    cancel = bc.cancelling_tail(logs[0], first_row, tail)
    assert commit_case(drivers, build, k, first_row, [cancel], [mm.mul(logs[0], mm.GENERATOR)], basis) == [None]
    holed = list(basis)
    holed[first_row + 2] = None
    holed[first_row + 4] = holed[first_row + 3]
    values = bc.commit_tail_values(tail, 1)[0]
    got = commit_case(drivers, build, k, first_row, [values], [None], holed)
    assert got == [bm.commit_tail(None, values, holed[first_row:])] and got[0] is not None


def test_the_driver_refuses_what_the_library_refuses(drivers):
    d = drivers.dir
    for name in ("tail.bin", "basis.bin", "commit.bin"):
        (d / name).write_bytes(b"")
    for k, n_cols, first_row in ((9, 1, 0), (10, 0, 1018), (10, 1, 959), (10, 1, 1024), (29, 1, 0)):
        assert drivers("commit", k, n_cols, first_row, d / "tail.bin", d / "basis.bin", d / "commit.bin", d / "out.bin") == ["refused"]
