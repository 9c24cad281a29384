"""The circuit search of the many-circuit checker (csrc/aesw_circ_search.h), compiled for the host: the code the kernel runs,
reached through aesw_circ_circuit_of_block of libaesw_circ.so (no GPU needed).

  * for valid offsets it is numpy.searchsorted(offsets, b, side="right") - 1 for EVERY block: empty circuits at the start, in
    the middle and at the end, runs of them, C = 1, C = 4 097, n = 0;
  * for ANY offsets -- random, decreasing, oversized, all-ones -- the circuit lies in [0, C) for every block below n.  The
    kernel forms every address from that circuit and a block index below n only, which is why broken offsets cannot move a
    read outside the batch (tests/test_gpu_circ_check.py counts them on the device; nothing there provokes a fault)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def search(pkg):
    lib = pkg.api.load_circ_library()

    def f(offsets, b):
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        return int(lib.aesw_circ_circuit_of_block(offs.ctypes.data_as(C.c_void_p), offs.size - 1, int(b)))
    return f


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


VALID = {
    "one-circuit": [7],
    "one-empty-circuit": [0],
    "empty-at-the-start": [0, 0, 3, 4],
    "empty-in-the-middle": [5, 0, 0, 0, 2, 0, 1],
    "empty-at-the-end": [3, 4, 0, 0],
    "empty-everywhere": [0, 2, 0, 0, 9, 1, 0, 1, 0],
    "all-empty": [0, 0, 0, 0, 0],
    "two": [1, 1],
    "full-circuits": [34] * 64,
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_every_block_finds_its_circuit(search, name):
    offs = _offsets(VALID[name])
    n = int(offs[-1])
    for b in range(n):
        exp = int(np.searchsorted(offs, b, side="right")) - 1
        assert search(offs, b) == exp, (name, b)
        assert offs[exp] <= b < offs[exp + 1]
    if n == 0:  # no block to look up; whatever is asked stays inside [0, C)
        assert 0 <= search(offs, 0) < len(offs) - 1


def test_4097_ragged_circuits(search):
    rng = np.random.default_rng(4097)
    counts = rng.integers(0, 11, 4097)
    counts[[0, 1, 2000, 2001, 4095, 4096]] = 0
    counts[17] = 10
    offs = _offsets(counts)
    n = int(offs[-1])
    exp = np.searchsorted(offs, np.arange(n, dtype=np.uint64), side="right") - 1
    got = np.array([search(offs, b) for b in range(n)])
    assert np.array_equal(got, exp)
    assert set(np.unique(got)) == set(np.nonzero(counts)[0])  # empty circuits are skipped, every other one is found


def test_package_wrapper(pkg):
    assert pkg.circuit_of_block([0, 0, 3, 3, 5], 2) == 1 and pkg.circuit_of_block([0, 0, 3, 3, 5], 3) == 3
    with pytest.raises(ValueError):
        pkg.circuit_of_block([0], 0)


@pytest.mark.parametrize("kind", ["random", "decreasing", "oversized", "ones", "first-nonzero", "last-short"])
def test_any_offsets_keep_the_circuit_inside_the_batch(search, kind):
    rng = np.random.default_rng(sum(kind.encode()))
    for nc in (1, 2, 3, 7, 64, 1000):
        n = 257
        if kind == "random":
            offs = rng.integers(0, 2 ** 63, nc + 1, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, nc + 1, dtype=np.uint64)
        elif kind == "decreasing":
            offs = np.sort(rng.integers(0, n + 1, nc + 1).astype(np.uint64))[::-1].copy()
        elif kind == "oversized":
            offs = _offsets(rng.integers(0, 2 ** 40, nc))
        elif kind == "ones":
            offs = np.full(nc + 1, 2 ** 64 - 1, dtype=np.uint64)
        elif kind == "first-nonzero":
            offs = _offsets(rng.integers(0, 5, nc)) + np.uint64(100)
        else:
            offs = _offsets(rng.integers(0, 3, nc)) // np.uint64(2)
        for b in list(range(n)) + [2 ** 40, 2 ** 64 - 1]:
            c = search(offs, b)
            assert 0 <= c < nc, (kind, nc, b, c)
