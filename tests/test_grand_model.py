"""The specification of libaesw_grand.so without a GPU.

csrc/aesw_grand.h -- the rules the kernels share: what an index reads, what a row multiplies Z by, Montgomery's batch inversion
with its skipped zero sums, the chunks of an argument and the workspace -- is compiled alone with g++
(tests/grand_rule_driver.cpp: no ROCm include, no GPU) and held against tests/grand_model.py.  The model itself is held against
halo2's statement: over the oracle's K = 14 / N = 3 circuit, with the input column of tests/theta_model.py and the permuted
columns tests/perm_model.py arranges from tests/mult_model.py's histogram, the closing product of an argument is 1, and it is
not 1 after one planted swap in A'."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grand_cases as gc
import grand_model as gm
import mult_model as mm
import perm_model as pm
import theta_model as tm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("grand_rule")
    exe = d / "grand_rule_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "grand_rule_driver.cpp"), "-o", str(exe)], check=True)

    def run(*args, cells=None):
        names = []
        if cells is not None:
            np.ascontiguousarray(cells, np.uint8).tofile(d / "in.bin")
            names = [str(d / "in.bin"), str(d / "out.bin")]
        out = subprocess.run([str(exe)] + [str(a) for a in args] + names, capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr)
        return out.stdout, (np.fromfile(d / "out.bin", np.uint8).reshape(-1, 32) if cells is not None else None)
    return run


def test_the_header_is_free_of_hip():
    text = (ROOT / "halo2-aes_amd" / "csrc" / "aesw_grand.h").read_text()
    assert "hip/" not in text and "asm" not in text.replace("assembly", "")


def test_an_index_behind_the_table_reads_the_all_zero_row_and_the_key_is_perms(driver):
    probes = (0, 1, 66559, 66560, 66561, 1 << 17, 0xFFFFFFFF, 7, 12)
    out, _ = driver("index", *probes)
    got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert [g[0] for g in got] == [int(v) for v in gm.row_of_index(np.array(probes))]
    assert [g[1] for g in got] == [(x // 5) * 8 + x % 5 + 1 for x in probes]  # set * 8 + tag of argument x = set * 5 + tag - 1


def test_the_row_rule_is_the_models(driver):
    rng = np.random.default_rng(0x6772)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % gm.R  # noqa: E731
    rows = [[rnd() for _ in range(6)] for _ in range(200)]
    rows += [[0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0], [gm.R - 1] * 6, [5, 6, 0, 9, 1, 2], [gm.R - 3, 6, 2, 9, 3, 2]]  # a zero inverse, a zero numerator
    _, got = driver("rows", cells=gm.cells([v for row in rows for v in row]))
    exp = gm.cells([(ti + b) * (tt + g) % gm.R * ia % gm.R * isv % gm.R for ti, tt, ia, isv, b, g in rows])
    assert np.array_equal(got, exp)
    assert not got[-1].any() and not got[-2].any()


@pytest.mark.parametrize("batch", (1, 3, 8, 16))
def test_the_batch_inversion_is_the_models_and_skips_zero_sums(driver, batch):
    rng = np.random.default_rng(0x6261 + batch)
    c = int.from_bytes(rng.bytes(40), "little") % gm.R
    x = [int.from_bytes(rng.bytes(40), "little") % gm.R for _ in range(8 * batch + 5)]  # the last batch is not full
    for at in (0, batch - 1, batch, 3 * batch + 1, len(x) - 1, 5 * batch, 5 * batch + 1):  # first and last of a batch, two in one, the tail
        x[at % len(x)] = (gm.R - c) % gm.R
    zeros = sum(1 for v in x if (v + c) % gm.R == 0)
    out, got = driver("batch", batch, cells=gm.cells([c] + x))
    assert zeros >= 5 and int(out) == zeros
    assert np.array_equal(got, gm.cells([gm.inv((v + c) % gm.R) for v in x]))
    # a batch of zero sums alone
    out, got = driver("batch", batch, cells=gm.cells([c] + [(gm.R - c) % gm.R] * (2 * batch)))
    assert int(out) == 2 * batch and not got.any()


def test_the_chunks_and_the_workspace(driver, pkg):
    lib = pkg.api.load_grand_library()
    for k, n_rows, n_sets in ((17, 66561, 1), (17, 66563, 2), (17, (1 << 17) - 6, 1), (17, 1 << 17, 1024), (17, 66560 + 1024, 1), (20, 1 << 20, 4), (30, 1 << 30, 1024),
                              (30, (1 << 30) - 1, 1)):
        last, chunks, stride, ws, rows_per_lane, batch = [int(v) for v in driver("geometry", k, n_rows, n_sets)[0].split()]
        chunk = 256 * rows_per_lane
        assert last == min(n_rows, (1 << k) - 1) and chunks == last // chunk + 1 and stride == (1 << k) // chunk and chunks <= stride
        assert ws == 5 * n_sets * (32 * stride + 16) and ws % 16 == 0 and ws == int(lib.aesw_grand_workspace_bytes(k, n_sets))
        assert rows_per_lane == 4 and batch in (4, 8, 16)  # the shipped form: never a lane-per-row inversion
    for k, n_sets in ((16, 1), (31, 1), (17, 0), (17, 1025), (0, 0)):
        assert int(driver("geometry", k, 66561, n_sets)[0].split()[3]) == 0 and int(lib.aesw_grand_workspace_bytes(k, n_sets)) == 0


@pytest.fixture(scope="module")
def circuit(oracle):
    k, n_sets, n = 14, 3, 31
    rng = np.random.default_rng(0x6772616e64)
    key, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
    with oracle.circuit(k, n_sets, key, pt, record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
    return adv, sel


def test_the_models_closing_product_is_one_for_permuted_columns_and_not_after_a_swap(oracle, circuit):
    adv, sel = circuit
    u, pad, st = 1 << 17, 0, 1  # the circuit's 2^14 rows, the all-zero row behind them: the arrangement needs room for the table
    theta, beta, gamma = gc.seeded(gc.THETA_SEED), gc.seeded(gc.CHALLENGE_SEEDS[0]), gc.seeded(gc.CHALLENGE_SEEDS[1])
    tables = [gm.values(t) for t in tm.compressed_tables(oracle.lookup_table(), theta)]
    column, _lookups, misses = tm.input_columns(adv, sel, oracle.tables())
    hist, _ = mm.multiplicities(adv, sel, oracle.tables())
    assert misses == 0
    for tag in (1, 2, 4):  # one argument of each table
        table = tables[gm.TABLE_OF_TAG[tag]]
        inputs = np.concatenate([column[st, tag - 1], np.full(u - column.shape[2], gm.ZERO_ROW)])
        a, s, over = pm.arrange(hist[st], tag, u, pad)
        assert not over
        z = gm.argument_product(table, inputs, a, s, beta, gamma, pad)
        assert len(z) == u + 1 and z[0] == 1 and z[u] == 1 and 0 not in z, tag
        assert gm.report([[z] * 5], u) == {"arguments": 5, "open": 0, "first_open": None}
        swapped = a.copy()
        swapped[0] = (int(swapped[0]) + 1) % gm.ZERO_ROW  # another row of the table in A'[0]: no permutation of the inputs any more
        z = gm.argument_product(table, inputs, swapped, s, beta, gamma, pad)
        assert z[u] != 1 and z[0] == 1, tag
        assert gm.report([[z] * 5], u) == {"arguments": 5, "open": 5, "first_open": (0, 1)}
