"""The specification of libaesw_msm.so without a GPU.

tests/msm_model.py -- bn256's G1 in Python integers -- is held against itself: the generator is on the curve and of order r, the
naive multi-scalar product and the commitment by known logarithms agree at n = 64.  csrc/aesw_msm.h -- the point forms, the one
addition law, the doubling, the windows, the slices and the chunks, the workspace -- is compiled alone with g++ into
tests/msm_driver.cpp, a program of its own that executes the digits, sort, bucket-walk, reduce and combine passes of
msm/aesw_msm.hip on the CPU through those functions, lane by lane, and is held against the model at k = 10 and 11, for cells and
bytes, with 1, 2 and 3 slices (and the rule's own count), once plain and once under -fsanitize=address,undefined.  The addition law
is held on every special pair: P + P, P + (-P), the identity on either side and on both, 2 P + P and (r - 1) G + G.  The group is of
odd prime order, so it has no point of order two and the complete formulas have no y-dependent case of their own in the doubling."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import msm_cases as mc
import msm_model as mm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("msm_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("msm_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "msm_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_msm.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text
    assert '#include "aesw_fq.h"' in text and '#include "aesw_fr.h"' in text and text.count("#include \"aesw") == 2  # the two fields alone


def test_the_model_is_a_group_of_order_r_and_its_two_oracles_agree():
    g = mm.GENERATOR
    assert mm.on_curve(g) and mm.on_curve(None) and not mm.on_curve((0, 0)) and mm.mul(mm.R, g) is None and mm.mul(mm.R - 1, g) == mm.neg(g)
    assert mm.add(g, mm.neg(g)) is None and mm.add(None, g) == g == mm.add(g, None) and mm.add(g, g) == mm.mul(2, g)
    scalars = mm.seeded_scalars(64, 0x6f72)
    basis = mm.known_basis(64)
    assert all(mm.on_curve(p) for p in basis) and basis[5] == mm.mul(mm.E0 + 5 * mm.D, g)
    assert mm.msm(scalars, basis) == mm.known_commit(scalars) and mm.known_commit(scalars) is not None
    assert mm.from_points(mm.to_points([None, g, basis[3]])) == [None, g, basis[3]]


def test_the_constants_and_the_sizes(drivers, pkg):
    chunk, threads, min_chunks, target = [int(v) for v in drivers("constants")[0].split()]
    lib = pkg.api.load_msm_library()
    assert chunk == int(lib.aesw_msm_chunk_rows()) and threads == 256 and chunk % (4 * threads) == 0 and target == 4096
    for k, n_cols, kind, slices in ((10, 1, mc.FR, 0), (10, 1, mc.BYTES, 3), (11, 3, mc.FR, 2), (16, 1, mc.BYTES, 0), (16, 1, mc.FR, 0), (20, 8, mc.FR, 0), (20, 1, mc.BYTES, 0),
                                    (28, 65535, mc.FR, 0), (10, 1, mc.FR, 64)):
        ws, sl, rows, chunks_first, chunks_last = [int(v) for v in drivers("sizes", k, n_cols, kind, slices)[0].split()]
        windows = 32 if kind == mc.FR else 1
        auto = max(1, min(-(-target // (windows * n_cols)), (1 << k) // (chunk * min_chunks)))
        assert sl == (slices or auto) == int(lib.aesw_msm_slices(k, n_cols, kind, slices))
        assert rows % 16 == 0 and rows * sl >= 1 << k and (rows - 16) * sl < 1 << k
        assert chunks_first == -(-min(rows, 1 << k) // chunk) and chunks_last <= chunks_first
        planes = (n_cols * 32 << k) if kind == mc.FR else 0
        assert ws == planes + 96 * n_cols * windows * (256 * sl + 1) == int(lib.aesw_msm_workspace_bytes(k, n_cols, kind, slices)) and ws % 16 == 0
    for k, n_cols, kind, slices in ((9, 1, 0, 0), (29, 1, 0, 0), (10, 0, 0, 0), (10, 65536, 0, 0), (10, 1, 2, 0), (10, 1, 0, 65), (28, 1, 1, 65536), (1 << 31, 1, 0, 0)):
        assert int(lib.aesw_msm_workspace_bytes(k, n_cols, kind, slices)) == 0 == int(lib.aesw_msm_slices(k, n_cols, kind, slices))
        assert drivers("sizes", k, n_cols, kind, slices)[0].split()[0] == "0"


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_addition_law_on_every_special_pair(drivers, build):
    d = drivers.dir
    p, q, r = mm.known_basis(3)
    double_p = mm.add(p, p)
    pairs = [(p, q), (p, p), (p, mm.neg(p)), (None, p), (p, None), (None, None), (double_p, p), (q, mm.neg(r)), (mm.GENERATOR, mm.GENERATOR),
             (mm.mul(mm.R - 1, mm.GENERATOR), mm.GENERATOR)]
    mm.to_points([a for a, _ in pairs]).tofile(d / "left.bin")
    mm.to_points([b for _, b in pairs]).tofile(d / "right.bin")
    drivers("law", d / "left.bin", d / "right.bin", d / "law.bin", build=build)
    got = mm.from_points(np.fromfile(d / "law.bin", np.uint8))
    for i, (a, b) in enumerate(pairs):
        full, mixed, doubled, swapped = got[4 * i:4 * i + 4]
        assert full == mixed == swapped == mm.add(a, b), (i, a, b)
        assert doubled == mm.add(a, a), (i, a)
    assert got[4 * 2] is None and got[4 * 5] is None  # P + (-P) and identity + identity are 64 zero bytes


@pytest.mark.parametrize("build", sorted(FLAGS))
@pytest.mark.parametrize("kind", (mc.FR, mc.BYTES), ids=mc.kind_name)
@pytest.mark.parametrize("k", mc.KS)
def test_the_cpu_run_of_the_passes_is_the_model(drivers, build, kind, k):
    d = drivers.dir
    mc.basis_cells(k).tofile(d / "basis.bin")
    # every column with three slices (an uneven last one); two of them with 1, 2 and the rule's count; under the sanitizers two, once
    runs = [(3, sorted(mc.columns(kind, k)))] + [(s, ["seeded", "ends"]) for s in (0, 1, 2)] if build == "plain" else [(3, ["seeded", "ends"])]
    for slices, names in runs:
        np.concatenate([mc.scalar_bytes(kind, mc.columns(kind, k)[name]).reshape(-1) for name in names]).tofile(d / "scalars.bin")
        drivers("commit", k, len(names), kind, slices, d / "scalars.bin", d / "basis.bin", d / "out.bin", build=build)
        got = np.fromfile(d / "out.bin", np.uint8).reshape(len(names), 64)
        for name, row in zip(names, got):
            assert row.tobytes() == mc.expected(kind, k, name).tobytes(), (k, kind, slices, name)
    assert not mc.expected(kind, k, "zero").any() and mc.expected(kind, k, "one").any()
    if build != "plain":
        return
    # a basis of one repeated point: every bucket adds P to P; a basis alternating P, -P under equal scalars passes through the identity
    p = mm.known_basis(1)[0]
    mm.to_points([p] * (1 << k)).tofile(d / "basis.bin")
    np.concatenate([mc.scalar_bytes(kind, mc.columns(kind, k)[name]).reshape(-1) for name in ("seeded", "same")]).tofile(d / "scalars.bin")
    drivers("commit", k, 2, kind, 2, d / "scalars.bin", d / "basis.bin", d / "out.bin", build=build)
    assert mm.from_points(np.fromfile(d / "out.bin", np.uint8)) == [mm.mul(sum(mc.columns(kind, k)[name]), p) for name in ("seeded", "same")]
    mm.to_points([p, mm.neg(p)] * (1 << (k - 1))).tofile(d / "basis.bin")
    drivers("commit", k, 2, kind, 3, d / "scalars.bin", d / "basis.bin", d / "out.bin", build=build)
    seeded = mc.columns(kind, k)["seeded"]
    assert mm.from_points(np.fromfile(d / "out.bin", np.uint8)) == [mm.mul(sum(seeded[0::2]) - sum(seeded[1::2]), p), None]
