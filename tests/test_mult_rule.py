"""The bin rule of the lookup multiplicities (csrc/aesw_mult.h) against the oracle's lookup table.  The header is compiled alone
with g++ -- no ROCm include, no GPU -- into tests/mult_rule_driver.cpp:

  * every row r of lookup_table() but the last is a hit whose bin is r, under the reference tables (S_BOX[255] = 23) and
    under the FIPS set;
  * whatever is no table row is a miss: for the one-operand tags exhaustively over (x, y) -- exactly 256 hits, each the table's
    --, for Xor every (x, y) with the right z hits and a wrong z, one per (x, y) and varied by a seed, never does;
  * tag 0 and numbers that are no tag have no bin and never hit;
  * the library's aesw_mult_bin is the header's;
  * the counter split of the kernels that count in LDS: every lookup is owned by exactly one half of a pair, its counter lies
    inside the half's counters, no two bins of a half share one, and the flush ranges of the two halves cover every bin but
    the zero row exactly once and map each counter back to the bin the index rule sent there."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as ol

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mult_rule") / "mult_rule_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "mult_rule_driver.cpp"), "-o", str(exe)], check=True)

    def ask(tables, commands):
        text = " ".join(str(int(v)) for v in np.concatenate(tables)) + "\n" + "\n".join(" ".join(str(v) for v in c) for c in commands)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(commands)
        return [[int(v) for v in line.split()] for line in out]
    return ask


TABLE_SETS = {"reference": lambda: ol.Oracle().tables(), "fips": lambda: ol.Oracle().fips_tables()}


@pytest.mark.parametrize("which", TABLE_SETS)
def test_every_table_row_is_a_hit_in_its_own_bin(driver, which):
    tables = TABLE_SETS[which]()
    t = ol.Oracle(tables).lookup_table()
    assert t.shape == (4, 66561) and not t[:, 66560].any()
    assert (int(tables[0][255]) == 23) == (which == "reference")
    got = driver(tables, [("r", *t[:, r]) for r in range(66560)])
    assert got == [[r, 1] for r in range(66560)]


@pytest.mark.parametrize("which", TABLE_SETS)
def test_what_is_no_table_row_is_a_miss(driver, which):
    tables = TABLE_SETS[which]()
    for tag in (3, 4, 5):
        assert driver(tables, [("m", tag)]) == [[256 * 4, 0]]  # 256 (x, y) pairs hit, under each of four z
    for seed in range(4):
        assert driver(tables, [("x", seed)]) == [[65536, 0]]
    # tag 0, and numbers that are no tag: no bin, no hit; a range lookup always hits and ignores y and z
    none = 2 ** 32 - 1
    assert driver(tables, [("r", 0, 5, 5, 0), ("r", 6, 1, 2, 3), ("r", 7, 0, 0, 0), ("r", 1, 200, 9, 9)]) == [[none, 0], [none, 0], [none, 0], [200, 1]]


def test_the_counter_split_and_the_flush_ranges_agree_bin_for_bin(driver):
    tables = ol.Oracle().tables()  # the split reads no table; the driver wants one
    once, over, clash, covered, stray, back = driver(tables, [("s",)])[0]
    assert once == 5 * 65536, "a lookup owned by both halves or by none"
    assert over == 0, "a counter index at or past XOR_HALF + SMALL"
    assert clash == 0, "two bins of one half on one counter"
    assert covered == 66560 and stray == 0, "the ranges cover bins 0 ... 66 559 exactly once and never the zero row"
    assert back == 0, "a range maps a counter to another bin than the index rule"


def test_the_library_exports_the_same_rule(pkg, driver):
    tables = ol.Oracle().tables()
    rng = np.random.default_rng(3)
    cases = [(int(t), int(x), int(y)) for t, x, y in zip(rng.integers(0, 8, 200), rng.integers(0, 256, 200), rng.integers(0, 256, 200))]
    got = driver(tables, [("r", t, x, y, 0) for t, x, y in cases])
    lib = pkg.api.load_mult_library()
    assert [int(lib.aesw_mult_bin(t, x, y)) for t, x, y in cases] == [g[0] for g in got]
    assert pkg.api.mult_bin(2, 1, 2) == 512 + 258 and pkg.api.mult_bin(0, 1, 2) is None
