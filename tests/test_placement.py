"""The placement rule (csrc/aesw_placement.h: which set and row a circuit gives its j-th block) against three references.  The
header is compiled alone with g++ -- no ROCm include, no GPU -- into tests/placement_driver.cpp, which answers for every K in
2 ... 20 with 1 ... 4 sets, and for K = 30 and 40 with 1 and 3 sets: the capacity, and (set, row) of every block (above K = 16
of the first, the last and the blocks on either side of a set boundary), through the 64-bit division and the 32-bit one.

  * the reference's rule (FixedAes128Config::aes_callable, src/aes128.rs:303-325), restated here as a walk over the sets: set 0
    gives up 1760 of its 2^K rows, every set then holds whole 1360-row blocks, set 0's behind its 400 key rows;
  * block_capacity / block_placement of the built library;
  * for K = 11 and 12 the rows at which the oracle's circuit (the restated synthesize()) places its blocks."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CASES = [(k, n_sets) for k in range(2, 21) for n_sets in range(1, 5)] + [(30, 1), (30, 3), (40, 1), (40, 3)]


def reference_sets(k, n_sets):
    """(first row, blocks) of every set, by the reference's rule."""
    sets = []
    for s in range(n_sets):
        max_row = 1 << k
        if s == 0:
            max_row -= 1760
        sets.append((400 if s == 0 else 0, max(max_row, 0) // 1360))
    return sets


def reference_place(sets, j):
    """(set, row) of block j, None past the last set."""
    for s, (first_row, blocks) in enumerate(sets):
        if j < blocks:
            return s, first_row + 1360 * j
        j -= blocks
    return None


def blocks_to_ask(k, sets):
    total = sum(b for _r, b in sets)
    if k <= 16:
        return list(range(total + 1))  # every block, and the first one past the end
    ask, b0 = {0, total - 1, total}, 0
    for _r, blocks in sets:
        ask |= {b0 - 1, b0}
        b0 += blocks
    return sorted(j for j in ask if 0 <= j <= total)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("placement") / "placement_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "placement_driver.cpp"), "-o", str(exe)], check=True)

    def ask(commands):
        text = "\n".join(" ".join(str(v) for v in c) for c in commands)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(commands)
        return [line.split() for line in out]
    return ask


@pytest.fixture(scope="module")
def header(driver):
    """(k, n_sets) -> (capacity, {j: ((set, row) by the 64-bit form, the same by the 32-bit form or None) or None past the end})"""
    commands = [("b", k, n_sets, j) for k, n_sets in CASES for j in blocks_to_ask(k, reference_sets(k, n_sets))]
    got = {}
    for (_b, k, n_sets, j), ans in zip(commands, driver(commands)):
        place = None
        if ans[1] != "-":
            place = ((int(ans[1]), int(ans[2])), None if ans[3] == "-" else (int(ans[3]), int(ans[4])))
        total, places = got.setdefault((k, n_sets), (int(ans[0]), {}))
        assert total == int(ans[0])
        places[j] = place
    return got


def test_header_is_the_reference_rule(header):
    assert sorted(header) == sorted(CASES)
    for (k, n_sets), (total, places) in header.items():
        sets = reference_sets(k, n_sets)
        assert total == sum(b for _r, b in sets), (k, n_sets)
        assert sorted(places) == blocks_to_ask(k, sets)
        for j, place in places.items():
            want = reference_place(sets, j)
            assert (place is None) == (want is None) == (j >= total), (k, n_sets, j)
            if place:
                assert place[0] == want, (k, n_sets, j)
                assert place[1] == (want if k <= 30 else None), (k, n_sets, j, "the 32-bit form")


@pytest.mark.parametrize("k,n_sets,cap0,capn,blocks", [
    pytest.param(9, 4, 0, 0, [], id="K=9: no block anywhere"),
    pytest.param(10, 4, 0, 0, [], id="K=10: no block anywhere"),
    pytest.param(11, 3, 0, 1, [(1, 0), (2, 0)], id="K=11: cap0=0 capn=1, block 0 sits in set 1"),
    pytest.param(12, 3, 1, 3, [(0, 400), (1, 0), (1, 1360), (1, 2720), (2, 0), (2, 1360), (2, 2720)], id="K=12: cap0=1 capn=3"),
])
def test_boundary_shapes(header, driver, k, n_sets, cap0, capn, blocks):
    assert driver([("c", k)]) == [[str(cap0), str(capn)]]
    total, places = header[(k, n_sets)]
    assert total == len(blocks)
    assert [places[j][0] for j in range(total)] == blocks and places[total] is None
    for n in range(1, 5):
        assert header[(k, n)][0] == cap0 + (n - 1) * capn
    if k == 9:
        assert all(header[(kk, n)][0] == 0 for kk in range(2, 11) for n in range(1, 5))


def test_filled_blocks_of_a_partly_filled_circuit(driver):
    """What the column checker's sweep asks: how many blocks of each set a circuit of n blocks fills, where the set starts."""
    commands = [("f", k, n_sets, n) for k, n_sets in CASES if k in (10, 11, 12, 16, 20, 30, 40)
                for n in sorted({0, 1, 2, *(sum(b for _r, b in reference_sets(k, n_sets)[:s]) + d for s in range(n_sets + 1) for d in (-1, 0, 1))}) if n >= 0]
    for (_f, k, n_sets, n), ans in zip(commands, driver(commands)):
        sets, b0, want = reference_sets(k, n_sets), 0, []
        for first_row, blocks in sets:
            want.append("%d:%d:%d" % (min(max(n - b0, 0), blocks), b0, first_row))
            b0 += blocks
        assert ans == want, (k, n_sets, n)


def test_library_places_blocks_as_the_header_does(pkg, header):
    for (k, n_sets), (total, places) in header.items():
        assert pkg.block_capacity(k, n_sets) == total, (k, n_sets)
        for j, place in places.items():
            if place:
                assert pkg.block_placement(k, n_sets, j) == place[0], (k, n_sets, j)
            else:
                with pytest.raises(pkg.AeswError) as e:
                    pkg.block_placement(k, n_sets, j)
                assert e.value.status == 5, (k, n_sets, j)  # AESW_ERR_CAPACITY


@pytest.mark.parametrize("k", [11, 12])
def test_oracle_circuit_places_blocks_at_the_same_rows(oracle, header, k):
    for n_sets in range(1, 5):
        total, places = header[(k, n_sets)]
        with oracle.circuit(k, n_sets, np.zeros(16, np.uint8), np.zeros((total, 16), np.uint8), record_copies=False) as c:
            assert c.status == 0
            assert [c.block_placement(j) for j in range(total)] == [places[j][0] for j in range(total)], (k, n_sets)
        with oracle.circuit(k, n_sets, np.zeros(16, np.uint8), np.zeros((total + 1, 16), np.uint8), record_copies=False) as c:
            assert c.status == 1  # one block more: the reference panics (src/aes128.rs:160-162)
