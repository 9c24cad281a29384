"""The host side of the column checker without a GPU: the hash that takes an Fr cell back to its byte
(aesw_cols_hash_search / _invert, the code the library runs when it is loaded) and the test model the GPU tests take their
expected reports from (tests/cols_model.py), held against the oracle's restated synthesize()."""
import ctypes as C

import numpy as np
import pytest

import cols_model as cm


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _search(lib, table):
    mul, bits, inv = C.c_uint32(), C.c_uint32(), np.zeros(4096, np.uint8)
    rc = lib.aesw_cols_hash_search(_p(table), C.byref(mul), C.byref(bits), _p(inv))
    return rc, mul.value, bits.value, inv


@pytest.mark.parametrize("which", ["bn256", "seeded"])
def test_the_hash_inverts_every_entry_and_rejects_every_single_bit_change(pkg, which):
    lib = pkg.api.load_cols_library()
    table = np.zeros((256, 32), np.uint8)
    lib.aesw_cols_fr_table(_p(table))
    assert np.array_equal(table, cm.fr_table())  # the table the library searched for is bn256's
    if which == "seeded":
        table = np.random.default_rng(0xC015).integers(0, 256, (256, 32), dtype=np.uint8)
    table = np.ascontiguousarray(table)
    rc, mul, bits, inv = _search(lib, table)
    assert rc == 0 and mul & 1 and 8 <= bits <= 12, (rc, mul, bits)
    if which == "bn256":
        assert bits == 8, bits  # a 256-byte inverse table is enough for the real one
    lo = table[:, :4].copy().view(np.uint32).reshape(256).astype(np.uint64)
    h = ((lo * mul) & 0xFFFFFFFF) >> (32 - bits)
    assert len(set(h.tolist())) == 256 and np.array_equal(inv[h], np.arange(256))
    for v in range(256):
        assert lib.aesw_cols_hash_invert(_p(table), mul, bits, _p(inv), _p(table[v])) == v
        for bit in range(256):
            cell = table[v].copy()
            cell[bit // 8] ^= 1 << (bit % 8)
            got = lib.aesw_cols_hash_invert(_p(table), mul, bits, _p(inv), _p(cell))
            assert got == -1, (v, bit, got)


@pytest.fixture(scope="module")
def k11(pkg, oracle):
    """A K = 11, N = 2 circuit (one block, in set 1) as the oracle's synthesize() lays it out, and the model over it."""
    k, n_sets = 11, 2
    assert pkg.block_capacity(k, n_sets) == 1
    rng = np.random.default_rng(1111)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    pt = rng.integers(0, 256, (1, 16), dtype=np.uint8)
    with oracle.circuit(k, n_sets, key, pt, record_copies=False) as c:
        assert c.num_advice == 7 and c.num_rows == 2048
        cols = np.stack([c.advice(j).astype(np.uint8) for j in range(7)])
        assigned = np.stack([c.advice_assigned(j).astype(bool) for j in range(7)])
        ct = c.ciphertext(0).reshape(1, 16)
    tab = np.concatenate([np.frombuffer(bytes(getattr(oracle.t, n)), np.uint8) for n in ("sbox", "mul2", "mul3")]).copy()
    m = cm.ColsModel(cm.load_lane_model(), tab, pkg, k, n_sets, [0, 1])
    return m, cols, assigned, pt, key.reshape(1, 16), ct


def test_the_model_is_satisfied_by_the_oracles_columns_in_both_forms(k11):
    m, cols, assigned, pt, keys, ct = k11
    assert np.array_equal(m.assigned(0), assigned)  # never-assigned, as the oracle's synthesize() has it
    assert not cols[~assigned].any()
    clean = {"blocks": 1, "keys": 1, "lookup_failures": 0, "copy_failures": 0, "gate_failures": 0, "input_failures": 0, "first": None,
             "offset_failures": 0, "cell_failures": 0, "unassigned_failures": 0, "first_cell": None, "cells": 7 * 2048, "satisfied": True}
    assert m.check(cols[None], pt, keys, ct) == clean
    assert m.check(m.lut[cols][None], pt, keys, ct) == clean
    assert m.check(cols[None], pt, None, None) == clean


def _regions(m, assigned):
    """name -> flat cell indices of every kind of region of the K = 11, N = 2 matrix."""
    idx = np.arange(assigned.size).reshape(assigned.shape)
    s, r = m.place[0]
    blk = slice(r, r + cm.AES_ROWS)
    reg = {}
    for col, name in enumerate("xyz"):
        a = assigned[3 * s + col, blk]
        reg["slab_" + name] = idx[3 * s + col, blk][a]
        if (~a).any():
            reg["slab_%s_unassigned" % name] = idx[3 * s + col, blk][~a]
        ka = assigned[col, :cm.KEY_ROWS]
        reg["key_" + name] = idx[col, :cm.KEY_ROWS][ka]
        if (~ka).any():
            reg["key_%s_unassigned" % name] = idx[col, :cm.KEY_ROWS][~ka]
        reg["tail_set0_" + name] = idx[col, cm.KEY_ROWS:]
        reg["tail_set1_" + name] = idx[3 * s + col, r + cm.AES_ROWS:]
    reg["words"] = idx[6, :cm.WORDS_ROWS]
    reg["words_tail"] = idx[6, cm.WORDS_ROWS:]
    assert sum(v.size for v in reg.values()) == assigned.size  # every cell is in exactly one region
    return reg


@pytest.mark.parametrize("form", ["bytes", "fr", "fr_noncanonical"])
def test_single_cell_changes_land_in_the_right_counter(k11, form):
    m, cols, assigned, pt, keys, ct = k11
    rng = np.random.default_rng({"bytes": 1, "fr": 2, "fr_noncanonical": 3}[form])
    reg = _regions(m, assigned)
    per = -(-2000 // len(reg))
    mat = cols.copy() if form == "bytes" else m.lut[cols]
    flat = mat.reshape(-1) if form == "bytes" else mat.reshape(-1, 32)
    done = 0
    for name, cells in reg.items():
        for i in rng.choice(cells, size=min(per, cells.size), replace=False):
            i = int(i)
            old = flat[i].copy()
            if form == "fr_noncanonical":
                bit = int(rng.integers(0, 256))
                flat[i, bit // 8] ^= 1 << (bit % 8)
            else:
                v = (int(cols.reshape(-1)[i]) ^ int(rng.integers(1, 256))) & 0xFF
                flat[i] = v if form == "bytes" else m.lut[v]
            got = m.check(mat[None], pt, keys, ct)
            flat[i] = old
            done += 1
            never = "unassigned" in name or "tail" in name
            assert not got["satisfied"], (name, i)
            assert got["unassigned_failures"] == (1 if never else 0), (name, i, got)
            assert got["cell_failures"] == (1 if form == "fr_noncanonical" else 0), (name, i, got)
            if never or form == "fr_noncanonical":
                assert got["first_cell"] == i, (name, i, got)
            else:
                assert got["first_cell"] is None
            if form != "fr_noncanonical":
                checks = sum(got[f] for f in cm.COUNTS)
                # a stray cell in a slab row nothing reads fails no check; an assigned cell always does
                assert (checks > 0) if not never else True, (name, i, got)
    assert done >= 2000, done
    assert m.check(mat[None], pt, keys, ct)["satisfied"]
