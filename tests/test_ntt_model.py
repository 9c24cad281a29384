"""The specification of libaesw_ntt.so without a GPU.

tests/ntt_model.py is held against the definition (sum a_i x^i by Horner at every point, k <= 8).  csrc/aesw_ntt.h -- zeta and 1/2
derived from the generator, the pass plan, the slot, twiddle and butterfly index functions, the tables, the workspace -- is
compiled alone with g++ into tests/ntt_driver.cpp, a program of its own that executes the plan on the CPU through those functions
with fr_mul, fr_add and fr_sub of aesw_fr.h, and is held against the model cell for cell: all four transforms at the smallest k
of one and of two passes (10 and NTT_PASS_LOG + 1 = 11, where the second pass has one stage), once plain and once under
-fsanitize=address,undefined.  Two full passes (k = 20) and the smallest k of three (21) are above what a model run follows
(k <= 18): there the driver transforms three coefficients and the rows are checked in closed form.  k = 28 is held by its plan
and by sampled slots of every pass alone."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ntt_cases as nc
import ntt_model as nm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("ntt_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("ntt_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "ntt_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def plain(hex_cell):
    return int(hex_cell, 16) * nm.MONT_INV % nm.R


def cell_hex(value):
    return "%064x" % (value * nm.MONT % nm.R)


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_ntt.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text


@pytest.mark.parametrize("k", range(1, 9))
def test_the_model_is_the_definition(k):
    n = 1 << k
    coeff = nm.seeded_values(n, 0x6e74 + k)
    w = nm.omega(k)
    assert nm.coeff_to_lagrange(coeff, k) == [nm.evaluate(coeff, pow(w, j, nm.R)) for j in range(n)]
    assert nm.lagrange_to_coeff(nm.coeff_to_lagrange(coeff, k), k) == coeff
    for sel in (0, 1):
        for ext_k in (k, k + 1, k + 3):
            ext = nm.coeff_to_extended(coeff, k, ext_k, sel)
            we = nm.omega(ext_k)
            assert ext == [nm.evaluate(coeff, nm.ZETAS[sel] * pow(we, j, nm.R) % nm.R) for j in range(1 << ext_k)]
            assert nm.extended_to_coeff(ext, ext_k, sel) == coeff + [0] * ((1 << ext_k) - n)


def test_the_constants_are_derived_and_are_the_models(drivers):
    lines = drivers("constants")
    assert int(lines[0]) == nc.PASS_LOG
    z0, z1, half = [plain(v) for v in lines[1:4]]
    assert (z0, z1) == nm.ZETAS and half == pow(2, -1, nm.R)
    assert ("%x" % z1).startswith("3064") and ("%x" % z1).endswith("636f23")  # the square; that halo2 calls THIS one Fr::ZETA is from memory, unpinned
    for k in (10, 14, 15, 28):
        w = plain(drivers("omega", k)[0])
        assert w == nm.omega(k) and pow(w, 1 << k, nm.R) == 1 and pow(w, 1 << (k - 1), nm.R) == nm.R - 1
    for k in (0, 10, 11, 17, 28):
        for v in (0, 1, 2):
            # 2^-k * zeta0^v in Montgomery form, as it lies in the tables
            assert int(drivers("scale", k, v)[0], 16) == pow(2, -k, nm.R) * pow(nm.ZETAS[0], v, nm.R) * nm.MONT % nm.R, (k, v)


def test_the_pass_plan_of_every_k(drivers):
    lines = drivers("plan")
    assert [int(line.split()[0]) for line in lines] == list(range(10, 29))
    P = nc.PASS_LOG
    for line in lines:
        k, passes, *rest = line.split()
        k, passes = int(k), int(passes)
        plan = [tuple(int(v) for v in r.split(":")) for r in rest]
        assert len(plan) == passes == -(-k // P)
        assert sum(m for _s0, m, _a in plan) == k and all(1 <= m <= P and a == P - m for _s0, m, a in plan)
        assert [s0 for s0, _m, _a in plan] == [sum(m for _s, m, _a in plan[:i]) for i in range(passes)]
        assert all(a <= s0 for s0, _m, a in plan[1:]) and plan[0][2] == 0  # a short pass finds its neighbours below s0
    by_k = {int(line.split()[0]): int(line.split()[1]) for line in lines}
    assert by_k[10] == 1 and by_k[P + 1] == 2 and by_k[2 * P] == 2 and by_k[nc.THREE_PASSES] == 3 and by_k[28] == 3


def test_the_table_and_workspace_sizes(drivers, pkg):
    lib = pkg.api.load_ntt_library()
    for max_k, k, n_cols in ((10, 10, 1), (13, 11, 3), (14, 14, 1), (15, 12, 5), (20, 17, 2), (28, 28, 16), (28, 22, 33), (28, 10, 65535)):
        tables, ws, low_at, high_at, scales_at, cells = [int(v) for v in drivers("sizes", max_k, k, n_cols)[0].split()]
        assert low_at == 1 << nc.PASS_LOG and high_at - low_at == 1 << min(max_k, 14) and scales_at - high_at == 1 << max(max_k - 14, 0) and cells - scales_at == 3 * 29
        assert tables == 32 * cells == int(lib.aesw_ntt_tables_bytes(max_k)) and tables <= 2 << 20
        assert ws == (0 if k <= nc.PASS_LOG else 32 * n_cols << k) == int(lib.aesw_ntt_workspace_bytes(k, n_cols)) and ws % 16 == 0
    for max_k in (0, 9, 29, 1 << 31):
        assert int(lib.aesw_ntt_tables_bytes(max_k)) == 0
    for k, n_cols in ((9, 1), (29, 1), (11, 0), (11, 65536)):
        assert int(lib.aesw_ntt_workspace_bytes(k, n_cols)) == 0 and int(drivers("sizes", 10, k, n_cols)[0].split()[1]) == 0


def test_every_pass_of_k_28_places_its_slots_as_the_plan_says(drivers):
    """position = hi * 2^(s0+m) + t * 2^s0 + lo with the tile's 2^a neighbours lowest; the load twiddle lo * bitrev_m(t)"""
    k, P = 28, nc.PASS_LOG
    rng = np.random.default_rng(0x6e7474)
    for p, (s0, m) in enumerate(((0, 10), (10, 10), (20, 8))):
        a = P - m
        for w, slot in [(0, 0), ((1 << (k - P)) - 1, (1 << P) - 1)] + [(int(rng.integers(1 << (k - P))), int(rng.integers(1 << P))) for _ in range(6)]:
            t, lo = slot >> a, ((w & ((1 << (s0 - a)) - 1)) << a) | (slot & ((1 << a) - 1))
            hi = w >> (s0 - a)
            position, twiddle = [int(v) for v in drivers("positions", k, p, w, slot)[0].split()]
            assert position == (hi << (s0 + m)) | (t << s0) | lo and position < 1 << k
            assert twiddle == lo * int(format(t, "0%db" % m)[::-1], 2) and twiddle < 1 << (s0 + m)


RUNS = (("c2l", 10, 10, 0, 10), ("l2c", 10, 10, 0, 12), ("c2l", 11, 11, 0, 11), ("l2c", 11, 11, 0, 13), ("c2e", 10, 10, 1, 10), ("c2e", 10, 11, 0, 12),
        ("c2e", 10, 13, 1, 13), ("e2c", 10, 10, 0, 10), ("e2c", 10, 11, 1, 11), ("e2c", 10, 12, 0, 15))


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_cpu_run_of_the_plan_is_the_model(drivers, build):
    for i, (name, k, ext_k, sel, max_k) in enumerate(RUNS):
        in_k = ext_k if name == "e2c" else k
        values = nm.seeded_values(1 << in_k, 0x72756e + i)
        exp = {"c2l": lambda: nm.coeff_to_lagrange(values, k), "l2c": lambda: nm.lagrange_to_coeff(values, k),
               "c2e": lambda: nm.coeff_to_extended(values, k, ext_k, sel), "e2c": lambda: nm.extended_to_coeff(values, ext_k, sel)}[name]()
        src, dst = drivers.dir / "in.bin", drivers.dir / "out.bin"
        nm.to_cells(values).tofile(src)
        drivers("run", name, k, ext_k, sel, max_k, src, dst, build=build)
        got = np.fromfile(dst, np.uint8).reshape(-1, 32)
        assert np.array_equal(got, nm.to_cells(exp)), (name, k, ext_k, sel, max_k)


@pytest.mark.parametrize("k,max_k,build", ((2 * nc.PASS_LOG, 20, "plain"), (nc.THREE_PASSES, 22, "plain"), (nc.PASS_LOG + 1, 11, "sanitized")))
def test_two_full_passes_and_three_passes_by_three_coefficients(drivers, k, max_k, build):
    n = 1 << k
    rng = np.random.default_rng(0x737061 + k)
    exps = (n - 1, int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1)))
    coeffs = nm.seeded_values(3, 0x636f + k)
    P = nc.PASS_LOG
    rows = sorted({0, n - 1, (1 << P) - 1, 1 << P, (1 << min(2 * P, k)) - 1, (1 << min(2 * P, k)) % n, n // 2} | {int(v) for v in rng.integers(0, n, 64)})
    args = [v for e, c in zip(exps, coeffs) for v in (e, cell_hex(c))]
    got = [plain(v) for v in drivers("sparse", k, max_k, *args, *rows, build=build)]
    w = nm.omega(k)
    assert got == [sum(c * pow(w, i * e, nm.R) for e, c in zip(exps, coeffs)) % nm.R for i in rows]


@pytest.mark.parametrize("k,ext_k,sel,build", ((18, 2 * nc.PASS_LOG, 0, "plain"), (19, nc.THREE_PASSES, 1, "plain"), (10, nc.PASS_LOG + 1, 1, "sanitized")))
def test_the_extended_transforms_over_two_full_and_three_passes_by_three_coefficients(drivers, k, ext_k, sel, build):
    """coeff_to_extended of sum c_j x^(e_j) is sum c_j zeta^(e_j mod 3) omega_ext^(i e_j) at row i -- the zero padding and the zeta cycle
    in the bit-reversed first load --, and extended_to_coeff of it is the three coefficients followed by zeros: the zeta scale in
    the last store."""
    n, ext_n = 1 << k, 1 << ext_k
    rng = np.random.default_rng(0x737865 + ext_k)
    exps = (n - 1, int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1)))
    assert len({e % 3 for e in exps} | {(exps[1] + 1) % 3}) >= 2
    coeffs = nm.seeded_values(3, 0x6578 + ext_k)
    P = nc.PASS_LOG
    rows = sorted({0, ext_n - 1, (1 << P) - 1, 1 << P, (1 << min(2 * P, ext_k)) - 1, (1 << min(2 * P, ext_k)) % ext_n, ext_n // 2} | {int(v) for v in rng.integers(0, ext_n, 64)})
    args = [v for e, c in zip(exps, coeffs) for v in (e, cell_hex(c))]
    lines = drivers("sparse_ext", k, ext_k, sel, ext_k, *args, *rows, build=build)
    w, z = nm.omega(ext_k), nm.ZETAS[sel]
    assert [plain(v) for v in lines[:-1]] == [sum(c * pow(z, e % 3, nm.R) * pow(w, i * e, nm.R) for e, c in zip(exps, coeffs)) % nm.R for i in rows]
    assert int(lines[-1]) == 0
