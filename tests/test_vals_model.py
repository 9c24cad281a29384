"""aesw_vals_check.h -- the values checker's own source -- on the CPU (tests/vals_model), against an independent expectation.

(1) The resolved table: 1 056 entries, 160 / 144 / 144 / 608 by tag, every operand a VALUES cell, a plaintext byte or a
round-key cell, every VALUES cell the output of exactly one entry, the rows those aesw_selector_tags enables a lookup on.
(2) tests/vals_recon.py fills the cells VALUES leaves out by copying along block_copy_graph; for oracle inputs the result is the
oracle's PACKED witness byte for byte.  (3) The model accepts the oracle's VALUES witness and catches EVERY single-byte change
of the 1 056 VALUES cells and the 936 key-slab cells; for each of them, and for changes of pt and ct bytes, its whole report
equals the report of the existing lane model (check_block / check_key) on the reconstructed PACKED witness."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from vals_recon import reconstruct

FIPS_B = (bytes.fromhex("3243f6a8885a308d313198a2e0370734"), bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"))
FIPS_C1 = (bytes.fromhex("00112233445566778899aabbccddeeff"), bytes.fromhex("000102030405060708090a0b0c0d0e0f"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def vmodel(pkg):
    import __graft_entry__ as ge
    L = C.CDLL(str(ge.build_vals_model()))
    L.vals_model_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 8
    L.vals_model_table.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def lmodel(pkg):
    import __graft_entry__ as ge
    L = C.CDLL(str(ge.build_lane_model()))
    L.lane_model_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 9
    return L


def _report(rep):
    f = int(rep[6])
    first = None if f == 2 ** 64 - 1 else (f >> 20, bool((f >> 19) & 1), (f >> 16) & 7, f & 0xFFFF)
    return {"blocks": int(rep[0]), "keys": int(rep[1]), "lookup": int(rep[2]), "copy": int(rep[3]), "gate": int(rep[4]),
            "input": int(rep[5]), "first": first}


def values_check(vmodel, tab, pt, keys, pbk, y, z, k, ct=None):
    rep = np.zeros(7, np.uint64)
    assert vmodel.vals_model_check(_p(tab), _p(pt), _p(keys), 1 if pbk else 0, pt.shape[0], _p(y), _p(z), _p(ct), _p(k.w), _p(k.kx),
                                   _p(k.ky), _p(k.kz), _p(rep)) == 0
    return _report(rep)


def packed_check(lmodel, tab, pt, keys, pbk, cols, k, ct=None):
    rep = np.zeros(7, np.uint64)
    x, y, z = cols
    assert lmodel.lane_model_check(_p(tab), ol.PACKED, _p(pt), _p(keys), 1 if pbk else 0, pt.shape[0], _p(x), _p(y), _p(z), _p(ct), _p(k.w),
                                   _p(k.kx), _p(k.ky), _p(k.kz), _p(rep)) == 0
    return _report(rep)


def _tab(oracle):
    return np.concatenate(oracle.tables()).copy()


def table_sets():
    rng = np.random.default_rng(0x7AB)
    ref = ol.Oracle()
    return {"reference": ref.tables(), "fips": ref.fips_tables(),
            "random": (rng.permutation(256).astype(np.uint8), rng.integers(0, 256, 256, dtype=np.uint8), rng.integers(0, 256, 256, dtype=np.uint8))}


def inputs(pbk, n_random=5, seed=11):
    """FIPS-197 appendix B and C.1, the block whose round-1 S-box input is 0xff in every byte, the zero vector, random blocks."""
    rng = np.random.default_rng(seed)
    pts = [np.frombuffer(FIPS_B[0], np.uint8), np.frombuffer(FIPS_C1[0], np.uint8), np.full(16, 0xFF, np.uint8), np.zeros(16, np.uint8)]
    keys = [np.frombuffer(FIPS_B[1], np.uint8), np.frombuffer(FIPS_C1[1], np.uint8), np.zeros(16, np.uint8), np.zeros(16, np.uint8)]
    pts += list(rng.integers(0, 256, (n_random, 16), dtype=np.uint8))
    keys += list(rng.integers(0, 256, (n_random, 16), dtype=np.uint8))
    pt = np.ascontiguousarray(np.stack(pts))
    return pt, (np.ascontiguousarray(np.stack(keys)) if pbk else np.zeros(16, np.uint8))  # shared: the zero key reaches S_BOX[0xff] in block 2


def test_the_resolved_table(pkg, vmodel):
    words, rows = np.zeros((1056, 2), np.uint32), np.zeros(1056, np.uint16)
    assert vmodel.vals_model_table(_p(words), _p(rows)) == 1056
    lw, lr = pkg.api.vals_check_table()  # the library's copy of the same
    assert np.array_equal(lw, words) and np.array_equal(lr, rows)
    lib = pkg.api.load_vals_library()
    assert lib.aesw_vals_check_rows() == 1056 and lib.aesw_vals_image_bytes() == 448 + 608 + 16 + 400 + 240 + 200 + 96 == vmodel.vals_model_image_bytes()
    ox, oy, oz, tag = words[:, 0] & 0xFFFF, words[:, 0] >> 16, words[:, 1] & 0xFFFF, words[:, 1] >> 16
    assert [int((tag == t).sum()) for t in (2, 3, 4, 5)] == [608, 144 + 16, 144, 144] and set(tag.tolist()) == {2, 3, 4, 5}
    etag = pkg.selector_tags()[0]
    assert np.array_equal(rows, np.nonzero(etag >= 2)[0]) and np.array_equal(tag, etag[rows])
    # the image: y [0, 448) | z [448, 1056) | pt [1056, 1072) | kx 400 | ky 240 | kz [1712, 1912) | words [1912, 2008)
    kzi = pkg.key_packed_index(2)
    round_key_cells = {1912 + i for i in range(16)} | {1712 + int(kzi[40 * r + 8 + i]) for r in range(10) for i in range(16)}
    assert len(round_key_cells) == 176
    allowed = set(range(1072)) | round_key_cells
    xor = tag == 2
    assert set(ox.tolist()) <= allowed and set(oy[xor].tolist()) <= allowed
    # outputs: y of a lookup row, z of an xor row -- each VALUES cell exactly once, where layout_index puts it
    iy, iz = pkg.layout_index(pkg.LAYOUT_VALUES, 1), pkg.layout_index(pkg.LAYOUT_VALUES, 2)
    assert np.array_equal(oy[~xor], iy[rows[~xor]]) and np.array_equal(oz[xor], 448 + iz[rows[xor]]) and np.all(oz[~xor] == 0xFFFF)
    outs = np.concatenate([oy[~xor], oz[xor]])
    assert sorted(outs.tolist()) == list(range(1056))
    # an operand never is the row's own output, and every plaintext byte and round-key cell is read
    assert np.all(ox != np.where(xor, oz, oy)) and np.all(oy[xor] != oz[xor])
    operands = set(ox.tolist()) | set(oy[xor].tolist())
    assert set(range(1056, 1072)) <= operands and round_key_cells <= operands


@pytest.mark.parametrize("tables", ["reference", "fips", "random"])
@pytest.mark.parametrize("pbk", [False, True])
def test_copying_along_the_graph_rebuilds_the_oracles_packed_witness(pkg, tables, pbk):
    o = ol.Oracle(tables=table_sets()[tables])
    pt, keys = inputs(pbk)
    v = o.encrypt_witness(pt, keys, layout=ol.VALUES)
    p = o.encrypt_witness(pt, keys, layout=ol.PACKED)
    k = o.key_schedule_witness(keys, layout=ol.PACKED)
    assert v.y.size == pt.shape[0] * 448 and v.z.size == pt.shape[0] * 608
    x, y, z = reconstruct(pkg, pt, v.y, v.z, (k.w, k.kx, k.ky, k.kz), pbk)
    assert np.array_equal(x, p.x) and np.array_equal(y, p.y) and np.array_equal(z, p.z)


@pytest.mark.parametrize("tables", ["reference", "fips", "random"])
@pytest.mark.parametrize("pbk", [False, True])
def test_an_oracle_witness_satisfies_the_values_check(vmodel, tables, pbk):
    o = ol.Oracle(tables=table_sets()[tables])
    tab = _tab(o)
    pt, keys = inputs(pbk, n_random=30)
    n = pt.shape[0]
    v, k = o.encrypt_witness(pt, keys, layout=ol.VALUES), o.key_schedule_witness(keys, layout=ol.PACKED)
    good = {"blocks": n, "keys": n if pbk else 1, "lookup": 0, "copy": 0, "gate": 0, "input": 0, "first": None}
    assert values_check(vmodel, tab, pt, keys, pbk, v.y, v.z, k, ct=v.ct) == good
    assert values_check(vmodel, tab, pt, keys if pbk else None, pbk, v.y, v.z, k) == good
    if tables != "reference":  # the tables are inputs of the check
        assert values_check(vmodel, _tab(ol.Oracle()), pt, keys, pbk, v.y, v.z, k, ct=v.ct)["lookup"] > 0


@pytest.mark.parametrize("pbk", [False, True])
def test_every_single_byte_change_is_caught_and_reported_as_the_packed_check_reports_it(pkg, vmodel, lmodel, oracle, pbk):
    tab = _tab(oracle)
    rng = np.random.default_rng(21 + pbk)
    n, blk = 3, 1
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16) if pbk else 16, dtype=np.uint8)
    v, k = oracle.encrypt_witness(pt, keys, layout=ol.VALUES), oracle.key_schedule_witness(keys, layout=ol.PACKED)
    ct = v.ct.copy()
    kslot = blk if pbk else 0

    def both():
        got = values_check(vmodel, tab, pt, keys, pbk, v.y, v.z, k, ct=ct)
        cols = reconstruct(pkg, pt, v.y, v.z, (k.w, k.kx, k.ky, k.kz), pbk)
        return got, packed_check(lmodel, tab, pt, keys, pbk, cols, k, ct=ct)

    got, want = both()
    assert got == want and got["first"] is None
    targets = [("y", v.y, blk * 448, 448), ("z", v.z, blk * 608, 608), ("pt", pt.reshape(-1), blk * 16, 16), ("ct", ct.reshape(-1), blk * 16, 16),
               ("kx", k.kx, kslot * 400, 400), ("ky", k.ky, kslot * 240, 240), ("kz", k.kz, kslot * 200, 200), ("w", k.w, kslot * 96, 96),
               ("keys", keys.reshape(-1), kslot * 16, 16)]
    missed, differ = [], []
    for name, arr, base, count in targets:
        for i in range(count):
            arr[base + i] ^= 1 << (i % 8)
            got, want = both()
            arr[base + i] ^= 1 << (i % 8)
            if got["first"] is None:
                missed.append((name, i))
            if got != want:
                differ.append((name, i, got, want))
            if name in ("y", "z", "pt", "ct"):
                assert got["copy"] == 0 and got["gate"] == 0 and got["first"][0] == blk and not got["first"][1], (name, i, got)
    assert not missed, missed[:10]
    assert not differ, differ[:3]
    got, want = both()
    assert got == want and got["first"] is None
