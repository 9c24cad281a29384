"""The specification of libaesw_theta.so without a GPU.

csrc/aesw_theta.h -- the rules the kernels share: tag -> table, what a table row compresses to, the row-order table index with
pad_row, the per-row input rule -- is compiled alone with g++ (tests/theta_rule_driver.cpp: no ROCm include, no GPU) and held
against tests/theta_model.py.  Over the oracle's K = 14 / N = 3 circuit the input column ties the new rule to the two merged
ones: per argument its bincount is the histogram section of tests/mult_model.py with the all-zero row taking the rest, and
sorted it is the A' tests/perm_model.py arranges from that histogram."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mult_model as mm
import oracle_lib
import perm_model as pm
import theta_model as tm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("theta_rule")
    exe = d / "theta_rule_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "theta_rule_driver.cpp"), "-o", str(exe)], check=True)

    def run(*args, files=None):
        names = []
        for i, a in enumerate(files or ()):
            if a is None:
                names.append("-")
            else:
                np.ascontiguousarray(a).tofile(d / ("in%d.bin" % i))
                names.append(str(d / ("in%d.bin" % i)))
        out = subprocess.run([str(exe)] + [str(a) for a in args] + names + [str(d / "out.bin")], capture_output=True, text=True)
        return out, d / "out.bin"
    return run


def test_the_header_is_free_of_hip():
    for name in ("aesw_theta.h", "aesw_fr.h"):
        text = (ROOT / "halo2-aes_amd" / "csrc" / name).read_text()
        assert "hip/" not in text and "asm" not in text.replace("assembly", ""), name


@pytest.mark.parametrize("tables", ("reference", "fips", "random"))
def test_the_compressed_tables_are_the_models(oracle, driver, tables):
    import guarded as G
    t = {"reference": oracle.tables, "fips": oracle.fips_tables, "random": G.random_tables}[tables]()
    table = oracle_lib.Oracle(tables=t).lookup_table()
    rng = np.random.default_rng(0x7461)
    thetas = (0, 1, tm.R - 1, int.from_bytes(rng.bytes(40), "little") % tm.R) if tables == "reference" else (int.from_bytes(rng.bytes(40), "little") % tm.R,)
    lut = tm.cells(range(256))
    for theta in thetas:
        out, path = driver("table", files=[np.concatenate(t), lut, tm.cells([theta])])
        assert out.returncode == 0, out.stderr
        raw = np.fromfile(path, np.uint8)
        got, of_tag = raw[:-5].reshape(3, tm.BINS, 32), raw[-5:]
        assert [int(v) for v in of_tag] == [tm.TABLE_OF_TAG[tag] for tag in tm.TAGS]
        exp = tm.compressed_tables(table, theta)
        assert np.array_equal(got, exp), (tables, theta, np.nonzero((got != exp).any(axis=2)))
        assert not got[:, tm.ZERO_ROW].any()
    out, path = driver("table", files=[np.concatenate(t), lut, np.frombuffer(tm.R.to_bytes(32, "little"), np.uint8)])
    assert out.returncode == 0 and not np.fromfile(path, np.uint8)[:-5].any()  # not canonical: the zero tables of the library


@pytest.mark.parametrize("tables", ("reference", "fips", "random"))
def test_a_table_row_is_the_lookup_tables_byte_for_byte(oracle, driver, tables):
    """theta_table_row derives a row from the sections of aesw_mult.h; the oracle writes load_enc_full_table() out row by row."""
    import guarded as G
    t = {"reference": oracle.tables, "fips": oracle.fips_tables, "random": G.random_tables}[tables]()
    out, path = driver("rows", files=[np.concatenate(t)])
    assert out.returncode == 0, out.stderr
    assert np.array_equal(np.fromfile(path, np.uint8).reshape(4, tm.BINS), oracle_lib.Oracle(tables=t).lookup_table())


def test_the_row_order_table_index(driver):
    for u, pad in ((66561, 0), (66563, 66560), (1 << 17, 7)):
        out, path = driver("index", u, pad)
        assert out.returncode == 0 and np.array_equal(np.fromfile(path, np.uint32), tm.table_column(u, pad))


@pytest.fixture(scope="module")
def circuit(oracle):
    k, n_sets, n = 14, 3, 31
    rng = np.random.default_rng(0x7468657461)
    key, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
    with oracle.circuit(k, n_sets, key, pt, record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
    return k, n_sets, n, key, pt, adv, sel


def test_the_models_input_column_is_the_histogram_and_sorts_to_a_prime(oracle, circuit):
    k, n_sets, n, _key, _pt, adv, sel = circuit
    column, lookups, misses = tm.input_columns(adv, sel, oracle.tables())
    hist, hist_misses = mm.multiplicities(adv, sel, oracle.tables())
    assert misses == 0 and hist_misses == 0 and lookups == 400 + 1056 * n
    for s in range(n_sets):
        for i, tag in enumerate(mm.TAGS):
            first, rows = mm.SECTIONS[i]
            col = column[s, tag - 1]
            counts = np.bincount(col, minlength=tm.BINS)
            section = hist[s][first:first + rows]
            assert np.array_equal(counts[first:first + rows], section), (s, tag)
            assert counts[tm.ZERO_ROW] == (1 << k) - section.sum() and counts.sum() == (1 << k), (s, tag)
            on = sel[5 * s + i] != 0
            assert (col[~on] == tm.ZERO_ROW).all()
            # the rows whose selector is on, sorted, then the all-zero row: A' of the merged arrangement, over u = 2^17 rows
            u = 1 << 17
            a, _t, over = pm.arrange(hist[s], tag, u, 0)
            assert not over and np.array_equal(a, np.concatenate([np.sort(col[on]), np.full(u - int(on.sum()), tm.ZERO_ROW)])), (s, tag)


@pytest.mark.parametrize("packed", (1, 0))
def test_the_headers_input_rule_is_the_model_on_the_oracles_circuit(oracle, driver, circuit, packed):
    k, n_sets, n, key, pt, adv, sel = circuit
    layout = oracle_lib.PACKED if packed else oracle_lib.DENSE
    w, kw = oracle.encrypt_witness(pt, key, layout=layout), oracle.key_schedule_witness(key, layout=layout)
    exp, lookups, _ = tm.input_columns(adv, sel, oracle.tables())
    out, path = driver("inputs", k, n_sets, n, packed, files=[np.concatenate(oracle.tables()), w.x, w.y, w.z, kw.kx, kw.ky, kw.kz])
    assert out.returncode == 0, out.stderr
    got = np.fromfile(path, np.uint32).reshape(n_sets, 5, 1 << k)
    assert np.array_equal(got, exp) and out.stdout.split() == [str(lookups), "0", str(2 ** 64 - 1)]
    # a planted miss: z of the xor row 20 of the circuit's last block; the cell alone changes, and the report names it
    z = w.z.copy()
    at = (n - 1) * (z.size // n) + (4 if packed else 20)  # row 20 is the fifth xor row of a block
    z[at] ^= 0x40
    out, path = driver("inputs", k, n_sets, n, packed, files=[np.concatenate(oracle.tables()), w.x, w.y, z, kw.kx, kw.ky, kw.kz])
    bad = np.fromfile(path, np.uint32).reshape(n_sets, 5, 1 << k)
    where = np.argwhere(bad != exp)
    assert where.shape == (1, 3) and bad[tuple(where[0])] == tm.MISS and where[0][1] == 1
    assert out.stdout.split() == [str(lookups), "1", str((n - 1) << 20 | 1 << 16 | 20)]
    # without a key slab the key rows read the all-zero row; beyond the capacity the rule is not asked
    out, path = driver("inputs", k, n_sets, n, packed, files=[np.concatenate(oracle.tables()), w.x, w.y, w.z, None, None, None])
    nokey = np.fromfile(path, np.uint32).reshape(n_sets, 5, 1 << k)
    sel0 = sel.copy()
    sel0[:5, :400] = 0
    assert np.array_equal(nokey, tm.input_columns(adv, sel0, oracle.tables())[0]) and out.stdout.split()[0] == str(lookups - 400)
