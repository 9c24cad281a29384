"""The specification of libaesw_perm.so without a GPU.

(1) csrc/aesw_perm.h -- the rule the kernels share -- is compiled alone with g++ (tests/perm_rule_driver.cpp: no ROCm include,
no GPU) and held position for position against tests/perm_model.py, which restates the construction with repeat and cumsum:
all five tags, u in {66 561, 66 564, 2^17 - 6, 2^17}, pad_row in {0, 66 560, a used row of the section}, and the histogram kinds
empty, one bin, all ones, sum exactly u, overflowing by 1 and by 2^20 -- every bin outside the section 0xffffffff.
(2) Independently of the construction, plookup's four relations are checked on the model's output by bincount and neighbour
comparison.  (3) Over the oracle's K = 14 / N = 3 circuit, used with k = 17, A' is the sorted multiset of the bins of the rows
whose selector is on, read off the assembled columns, padded with the all-zero row."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mult_model as mm
import perm_model as pm

ROOT = Path(__file__).resolve().parent.parent
US = (66561, 66564, (1 << 17) - 6, 1 << 17)
KINDS = ("empty", "one_bin", "all_ones", "exact", "over1", "over_big")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("perm_rule")
    exe = d / "perm_rule_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "perm_rule_driver.cpp"), "-o", str(exe)], check=True)

    def run(hist, tag, cases):
        """cases: (u, pad_row) pairs -> [(a, s, scalars)]"""
        np.asarray(hist, np.uint32).tofile(d / "hist.bin")
        args = [str(v) for case in cases for v in case]
        out = subprocess.run([str(exe), str(d / "hist.bin"), str(d / "out.bin"), str(tag)] + args, capture_output=True, text=True, check=True).stdout
        words, res, at = np.fromfile(d / "out.bin", np.uint32), [], 0
        for (u, _pad), line in zip(cases, out.splitlines()):
            res.append((words[at:at + u], words[at + u:at + 2 * u], [int(v) for v in line.split()]))
            at += 2 * u
        assert at == words.size and len(res) == len(cases)
        return res
    return run


def pads(hist, tag):
    """0, the all-zero row, and a row of the section with a count (an empty section: its first row)"""
    first, n = pm.SECTION[tag]
    used = np.nonzero(hist[first:first + n])[0]
    return (0, pm.ZERO_ROW, first + int(used[len(used) // 2]) if used.size else first)


@pytest.mark.parametrize("tag", pm.TAGS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_header_is_the_model_and_the_model_keeps_the_relations(driver, kind, tag):
    rng = np.random.default_rng(1000 * tag + KINDS.index(kind))
    for u in US:
        hist = pm.synthetic(kind, tag, u, rng)
        cases = [(u, pad) for pad in pads(hist, tag)]
        for (u, pad), (a, s, scalars) in zip(cases, driver(hist, tag, cases)):
            ea, es, over = pm.arrange(hist, tag, u, pad)
            at = (kind, tag, u, pad)
            assert over == kind.startswith("over"), at
            assert np.array_equal(a, ea), (at, np.nonzero(a != ea)[0][:5])
            assert np.array_equal(s, es), (at, np.nonzero(s != es)[0][:5])
            c, _ = pm.counts(hist, tag, u)
            first, n = pm.SECTION[tag]
            assert scalars == [u - c[pm.ZERO_ROW], int((c[first:first + n] > 0).sum()), int(c[pm.ZERO_ROW] > 0), int(over)], at
            # the relations, on the model's output and without its construction
            if not over:  # the inputs are the histogram's as it stands
                inputs = np.zeros(pm.BINS, np.int64)
                inputs[first:first + n] = hist[first:first + n]
                inputs[pm.ZERO_ROW] = u - inputs.sum()
                assert np.array_equal(inputs, c), at
            assert pm.relations(ea, es, c, u, pad) is None, at


def test_the_relations_check_sees_what_breaks_them():
    rng = np.random.default_rng(7)
    u, tag, pad = 66564, 3, 0
    hist = pm.synthetic("random", tag, u, rng)
    a, s, _ = pm.arrange(hist, tag, u, pad)
    c, _ = pm.counts(hist, tag, u)
    assert pm.relations(a, s, c, u, pad) is None
    i = int(np.nonzero(a[1:] != a[:-1])[0][0]) + 1  # the first position of a run
    for what, (ba, bs) in {"A'": (np.roll(a, 1), s), "S'": (a, np.where(np.arange(u) == u - 1, 5, s)), "neither": (a, np.concatenate([s[:i], s[i:][::-1]]))}.items():
        assert pm.relations(ba, bs, c, u, pad) is not None, what
    assert pm.relations(a, s, c, u, 1) is not None  # another pad row: another table column


@pytest.mark.parametrize("tables", ("reference", "fips"))
def test_a_real_circuit_sorts_to_the_models_input_column(oracle, driver, tables):
    import oracle_lib
    k, n_sets, n, u = 14, 3, 31, 1 << 17
    orc = oracle if tables == "reference" else oracle_lib.Oracle(tables=oracle.fips_tables())
    rng = np.random.default_rng(0x7065726D)
    with orc.circuit(k, n_sets, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8), record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
    hist, misses = mm.multiplicities(adv, sel, orc.tables())
    assert misses == 0
    for s in range(n_sets):
        for i, tag in enumerate(mm.TAGS):
            on = np.nonzero(sel[5 * s + i])[0]
            x, y = adv[3 * s][on].astype(np.int64), adv[3 * s + 1][on].astype(np.int64)
            bins = mm.SECTIONS[i][0] + (256 * x + y if tag == 2 else x)
            column = np.concatenate([np.sort(bins), np.full(u - bins.size, pm.ZERO_ROW, np.int64)])
            a, t, over = pm.arrange(hist[s], tag, u, 0)
            assert not over and np.array_equal(a, column), (s, tag)
            assert pm.relations(a, t, np.bincount(column, minlength=pm.BINS), u, 0) is None, (s, tag)
    (a, t, _), = driver(hist[1], 2, [(u, 0)])
    ea, et, _ = pm.arrange(hist[1], 2, u, 0)
    assert np.array_equal(a, ea) and np.array_equal(t, et)
