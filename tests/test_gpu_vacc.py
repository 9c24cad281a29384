"""libaesw_vacc.so / MultiplicityAccumulator.add_values on the GPU: the lookup multiplicities of one circuit accumulated from a
VALUES witness (tests/vacc_cases.py).  The yardstick is tests/mult_model.py over the ORACLE's circuit, as in tests/test_gpu_acc.py
(its expected()); where bytes are corrupted, mult_model over the columns assembled from the PACKED witness that
tests/vals_recon.py rebuilds from the corrupted bytes by copying.  Never a count of the product's.  d_mult and the report always
lie in poisoned, guard-banded buffers (tests/guarded.py): a call must touch nothing else.  Every corruption is planted in data."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as G
import mult_model as mm
import vacc_cases as vc
from test_gpu_acc import check_many_sets, expected, many_sets_expectation, same, untouched, worlds  # noqa: F401  (the oracle's circuits, computed once, and the fixture)
from vals_recon import reconstruct

pytestmark = pytest.mark.gpu

BINS = mm.BINS
OK, INVALID, CAPACITY = 0, 1, 5
YS, ZS = 448, 608
ROOT = Path(__file__).resolve().parent.parent


class Circuit:
    """One circuit on the device: n blocks under one key as a VALUES and as a PACKED witness, and the key's packed slab."""

    def __init__(self, pkg, ctx, k, n_sets, n, seed=0, identical=False):
        import torch
        self.pkg, self.ctx, self.k, self.n_sets, self.n = pkg, ctx, k, n_sets, n
        rng = np.random.default_rng(seed)
        self.key = rng.integers(0, 256, 16, dtype=np.uint8)
        self.pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        if identical:
            self.pt[:] = self.pt[0]
        self.d_key, self.d_pt = torch.from_numpy(self.key).cuda(), torch.from_numpy(self.pt).cuda()
        self.kw = ctx.key_schedule_witness(self.d_key.reshape(1, 16), vc.PACKED, want_rk=False)
        self.vals = ctx.encrypt_witness(self.d_pt, self.d_key, vc.VALUES) if n else ctx.alloc_witness(1, vc.VALUES)
        self.packed = ctx.encrypt_witness(self.d_pt, self.d_key, vc.PACKED) if n else ctx.alloc_witness(1, vc.PACKED)
        self.pst = [pkg.column_stride(vc.PACKED, i) for i in range(3)]
        assert [pkg.column_stride(vc.VALUES, i) for i in range(3)] == [0, YS, ZS]
        torch.cuda.synchronize()

    def values(self, first, count):
        """(pt, y, z) views of blocks [first, first + count)"""
        return self.d_pt[first:first + count], self.vals.y[first * YS:(first + count) * YS], self.vals.z[first * ZS:(first + count) * ZS]

    def packed_slabs(self, first, count):
        return [t[first * s:(first + count) * s] for t, s in zip(self.packed[:3], self.pst)]


class Acc:
    """The C ABI of both libraries on torch's current stream over one guarded histogram buffer and one guarded report."""

    def __init__(self, circ, arena, tag=""):
        import torch
        api = circ.pkg.api
        self.c, self.arena, self.alib, self.vlib = circ, arena, api.load_acc_library(), api.load_vacc_library()
        self.mult = arena.out("mult" + tag, circ.n_sets * BINS * 4)
        self.rep = arena.out("report" + tag, 24)
        assert untouched(arena, self.mult, self.rep)
        self.mult32 = self.mult.view(torch.int32).view(circ.n_sets, BINS)

    def _done(self, rc, expect):
        ctx = self.c.ctx
        assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
        return rc

    def reset(self):
        c = self.c
        return self._done(self.alib.aesw_acc_reset_device(c.ctx._h, c.n_sets, self.mult.data_ptr(), self.rep.data_ptr(), c.ctx._stream()), OK)

    def add(self, first, count, chunk=0, bufs=None, expect=OK, k=None, h=None, key="slab", mult=None, rep=None):
        """aesw_vacc_add_device_chunk; bufs = (pt, y, z) instead of the circuit's own; key: "slab", None (NULL) or a KeyWitness"""
        c = self.c
        pt, y, z = c.values(first, count) if bufs is None else bufs
        kw = c.kw if key == "slab" else key
        ks = None if kw is None else c.pkg.api.KeySlab(kw[0].data_ptr(), None, None, kw[3].data_ptr())  # kx and ky are not read
        return self._done(self.vlib.aesw_vacc_add_device_chunk(
            c.ctx._h if h is None else h, c.k if k is None else k, c.n_sets, first, count, pt.data_ptr(), y.data_ptr(), z.data_ptr(),
            None if ks is None else C.byref(ks), (self.mult if mult is None else mult).data_ptr(), (self.rep if rep is None else rep).data_ptr(),
            c.ctx._stream(), chunk), expect)

    def add_packed(self, first, count):
        c = self.c
        x, y, z = c.packed_slabs(first, count)
        return self._done(self.alib.aesw_acc_add_device(c.ctx._h, c.k, c.n_sets, first, count, vc.PACKED, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                                        self.mult.data_ptr(), self.rep.data_ptr(), c.ctx._stream()), OK)

    def add_key(self):
        c = self.c
        ks = c.pkg.api.KeySlab(None, *[t.data_ptr() for t in c.kw[1:4]])
        return self._done(self.alib.aesw_acc_add_key_device(c.ctx._h, c.k, vc.PACKED, C.byref(ks), self.mult.data_ptr(), self.rep.data_ptr(),
                                                            c.ctx._stream()), OK)

    def result(self):
        """(hist int64 [n_sets, BINS], report dict), guards checked"""
        import torch
        torch.cuda.synchronize()
        self.arena.check()
        return self.mult32.cpu().numpy().astype(np.int64), self.c.pkg.api.mult_report_dict(self.rep.view(torch.int64))


def clean(k, n, key=True):
    return {"lookups": (400 if key and k >= 9 else 0) + 1056 * n, "misses": 0, "first_miss": None}


@pytest.mark.parametrize("tables", vc.TABLE_SETS)
@pytest.mark.parametrize("k,n_sets,n", vc.SHAPES)
def test_every_cut_of_a_values_circuit_equals_the_model(pkg, worlds, k, n_sets, n, tables):
    import torch
    ctx, orc = worlds[tables]
    assert n <= pkg.block_capacity(k, n_sets)
    c = Circuit(pkg, ctx, k, n_sets, n, seed=k * 10 + n_sets)
    exp, exp_blocks = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    runs = vc.ragged(n)
    arenas = [G.DeviceArena(canary) for canary in G.CANARIES]

    a = Acc(c, arenas[0], "_whole")  # the whole circuit in one add
    a.reset(), a.add(0, n), a.add_key()
    got, rep = a.result()
    same(got, exp, "one add")
    assert rep == clean(k, n), rep

    for name, order in (("ragged", runs), ("reversed", runs[::-1])):  # the key slab first, once, and last
        a = Acc(c, arenas[1], "_" + name)
        a.reset()
        if name == "ragged":
            a.add_key()
        for first, count in order:
            a.add(first, count)
        if name == "reversed":
            a.add_key()
        got, rep = a.result()
        same(got, exp, name)
        assert rep == clean(k, n), rep

    # the same adds out of ONE y / z / pt buffer: generate, add, overwrite
    a = Acc(c, arenas[0], "_reuse")
    a.reset()
    longest = max([count for _f, count in runs] + [1])
    buf = ctx.alloc_witness(longest, vc.VALUES)
    ptbuf = torch.empty((longest, 16), dtype=torch.uint8, device="cuda")
    for first, count in runs:
        ptbuf[:count].copy_(c.d_pt[first:first + count])
        ctx.encrypt_witness(ptbuf[:count], c.d_key, vc.VALUES, out=buf)
        a.add(first, count, bufs=(ptbuf, buf.y, buf.z))
    got, rep = a.result()
    same(got, exp_blocks, "one buffer")
    assert rep == clean(k, n, key=False), rep

    # several pairs of workgroups add into the same bins; from LONG_FROM blocks on also chunks longer than one round of the waves
    for chunk in vc.FORCED_CHUNKS + (vc.LONG_CHUNKS if n >= vc.LONG_FROM else ()):
        a = Acc(c, arenas[1], "_chunk%d" % chunk)
        a.reset(), a.add_key(), a.add(0, n, chunk=chunk)
        got, rep = a.result()
        same(got, exp, "chunk %d" % chunk)
        assert rep == clean(k, n), rep

    if n >= 24:  # VALUES adds, PACKED adds of the other blocks and the key add into one histogram
        for values_first in (True, False):
            a = Acc(c, arenas[0], "_mixed%d" % values_first)
            a.reset()
            for i, (first, count) in enumerate(runs if values_first else runs[::-1]):
                (a.add if (i % 2 == 0) == values_first else a.add_packed)(first, count)
                if i == 1:
                    a.add_key()
            got, rep = a.result()
            same(got, exp, "VALUES and PACKED adds mixed")
            assert rep == clean(k, n), rep

    if (k, n_sets) == (14, 3):  # the Python face, on an accumulator made for PACKED witnesses
        acc = ctx.multiplicity_accumulator(k, n_sets)
        acc.reset()
        for first, count in runs[:-1]:
            pt, y, z = c.values(first, count)
            acc.add_values(first, pt, pkg.Witness(c.vals.x, y, z, None, None), c.kw)
        first, count = runs[-1]  # a larger buffer, partly used; then a PACKED add of nothing and the key
        acc.add_values(first, c.d_pt[first:], pkg.Witness(None, c.vals.y[first * YS:], c.vals.z[first * ZS:], None, None), c.kw, n_blocks=count, _chunk=3)
        acc.add(0, pkg.Witness(*c.packed_slabs(0, 1), None, None), n_blocks=0).add_key(c.kw)
        assert acc.report() == clean(k, n)
        same(acc.histograms().cpu().numpy().astype(np.int64), exp, "MultiplicityAccumulator.add_values")
        with pytest.raises(ValueError):
            acc.add_values(0, c.d_pt[:2], pkg.Witness(None, c.vals.y[:YS], c.vals.z[:ZS], None, None), c.kw, n_blocks=2)
    torch.cuda.synchronize()


def test_identical_blocks_count_exactly(pkg, worlds):
    """Every block the same: all workgroups add to the same few hundred words."""
    ctx, orc = worlds["reference"]
    k, n_sets, n, chunk = vc.CONTENTION
    c = Circuit(pkg, ctx, k, n_sets, n, seed=5, identical=True)
    exp, _ = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    assert np.count_nonzero(exp[1]) <= 1056 and exp[1].max() >= 12
    a = Acc(c, G.DeviceArena())
    a.reset(), a.add(0, n, chunk=chunk), a.add_key()
    got, rep = a.result()
    same(got, exp, "identical blocks")
    assert rep == clean(k, n)


def test_a_circuit_of_1024_sets(pkg, worlds):
    """n_sets at its bound: runs that start and end deep inside the set index, each add out of pt / y / z views of its own."""
    ctx, orc = worlds["reference"]
    k, n_sets = vc.MANY_SETS
    assert pkg.block_capacity(k, n_sets) == 3070
    c = Circuit(pkg, ctx, k, n_sets, 16, seed=1024)
    exp = many_sets_expectation(pkg, orc, c.key, c.pt)
    a = Acc(c, G.DeviceArena(), "_many")
    a.reset()
    at = 0
    for first, count in vc.MANY_RUNS:
        a.add(first, count, bufs=c.values(at, count))  # block first + i of a run is entry i of its buffers
        at += count
    check_many_sets(a, exp, 16)


def rebuilt_expectation(pkg, ctx, c, pt, y, z, kw_np):
    """(hist of the blocks, report) by mult_model over the columns the product assembles from the PACKED witness that copying
    rebuilds from these bytes; the key rows masked out.  The first miss: the smallest (block, slab row) whose row misses."""
    import torch
    k, n_sets, n = c.k, c.n_sets, c.n
    cols = reconstruct(pkg, pt, y, z, kw_np, False)
    wit = pkg.Witness(*[torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in cols], None, None)
    kw = pkg.KeyWitness(*[torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in kw_np], None)
    adv = ctx.assemble_advice_circuits(k, n_sets, wit, kw, [n], as_fr=False, layout=vc.PACKED, n_blocks=n).cpu().numpy()[0]
    sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
    sel = np.asarray(sel).copy()
    sel[:5, :pkg.KEY_ROWS] = 0
    hist, misses = mm.multiplicities(adv, sel, ctx._tables)
    first = None
    for b in range(n):
        s, row = pkg.block_placement(k, n_sets, b)
        a3, s5 = adv[3 * s:3 * s + 3, row:row + 1360], sel[5 * s:5 * s + 5, row:row + 1360]
        pad = np.zeros((1, 1360), np.uint8)

        def missed(j):  # over the block's first j rows
            return mm.multiplicities(np.concatenate([a3[:, :j], pad[:, :j]]), np.concatenate([s5[:, :j], pad[:, :j]]), ctx._tables)[1]
        if missed(1360):
            lo, hi = 0, 1360  # missed(lo) == 0 < missed(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if missed(mid) else (mid, hi)
            first = (b, False, hi - 1)
            break
    return hist, {"lookups": 1056 * n, "misses": misses, "first_miss": first}


@pytest.mark.parametrize("what", vc.CORRUPTIONS)
def test_corrupted_bytes_count_as_the_rebuilt_packed_witness_counts(pkg, worlds, what):
    import torch
    ctx, _orc = worlds["reference"]
    k, n_sets, n = 14, 3, 34
    c = Circuit(pkg, ctx, k, n_sets, n, seed=77)
    words, rows = pkg.api.vals_check_table()
    ox, oy, tag = words[:, 0] & 0xFFFF, words[:, 0] >> 16, words[:, 1] >> 16
    y_read_later = sorted(set(oy[tag == 3].tolist()) & set(ox.tolist()))  # the output of an S-box row that later rows read
    kz_read = sorted({int(o) - 1712 for o in np.concatenate([ox, oy]) if 1712 <= o < 1912})
    assert len(y_read_later) >= 100 and len(kz_read) == 160
    if "y" in what:
        c.vals.y[5 * YS + y_read_later[37]] ^= 0x40
    if "z" in what and what != "kz":
        c.vals.z[20 * ZS + 77] ^= 0x01
    if what == "pt":
        c.d_pt[30, 3] ^= 0x80
    if what == "kz":
        c.kw.kz[kz_read[40]] ^= 0x04
    torch.cuda.synchronize()
    kw_np = tuple(t.cpu().numpy() for t in c.kw[:4])
    want, want_rep = rebuilt_expectation(pkg, ctx, c, c.d_pt.cpu().numpy(), c.vals.y.cpu().numpy(), c.vals.z.cpu().numpy(), kw_np)
    # the own row of a corrupted cell misses, and so may every row that reads it
    at_least = {"y": 2, "z": 1, "pt": 1, "kz": n, "y+z": 3}[what]
    assert want_rep["misses"] >= at_least and int(want.sum()) == 1056 * n - want_rep["misses"]
    assert want_rep["first_miss"][0] == {"y": 5, "z": 20, "pt": 30, "kz": 0, "y+z": 5}[what]
    runs = vc.ragged(n)
    for order, chunk, canary in ((runs, 0, G.CANARIES[0]), (runs[::-1], 3, G.CANARIES[1])):
        a = Acc(c, G.DeviceArena(canary), "_" + what)
        a.reset()
        for first, count in order:
            a.add(first, count, chunk=chunk)
        got, rep = a.result()
        same(got, want, what)
        assert rep == want_rep, (rep, want_rep)


def test_captured_calls_replay_and_captured_adds_accumulate(pkg, worlds):
    import torch
    ctx, orc = worlds["reference"]
    k, n_sets, n = 14, 3, 34
    c = Circuit(pkg, ctx, k, n_sets, n, seed=14)
    exp, exp_blocks = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    assert pkg.api.load_vacc_library().aesw_vacc_prepare(ctx._h) == OK  # the one synchronous step, ahead of the capture
    arena = G.DeviceArena()
    adds = ((0, 9), (9, 14), (23, 11))

    a = Acc(c, arena, "_all")  # reset + 3 adds + add_key: every replay gives the same
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        a.reset()
        for first, count in adds:
            a.add(first, count)
        a.add_key()
    torch.cuda.synchronize()
    assert untouched(arena, a.mult, a.rep), "the captured calls ran during capture"
    for i in range(3):
        graph.replay()
        got, rep = a.result()
        same(got, exp, "replay %d" % i)
        assert rep == clean(k, n)

    b = Acc(c, arena, "_adds")  # the adds alone, twice after one reset: exactly twice the model
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=torch.cuda.Stream()):
        for first, count in adds:
            b.add(first, count)
    torch.cuda.synchronize()
    assert untouched(arena, b.mult, b.rep)
    b.reset()
    graph2.replay()
    graph2.replay()
    got, rep = b.result()
    same(got, 2 * exp_blocks, "two replays of the adds")
    assert rep == {"lookups": 2 * 1056 * n, "misses": 0, "first_miss": None}


def test_refusals_leave_the_outputs_alone_and_say_why(pkg, worlds):
    import torch
    ctx, _orc = worlds["reference"]
    c = Circuit(pkg, ctx, 12, 2, 3, seed=3)
    arena = G.DeviceArena()
    a = Acc(c, arena)
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    assert a.add(0, 3, key=None, expect=INVALID) == INVALID and "aesw_vacc_add_device" in err() and "d_key_slab" in err()
    pt, y, z = c.values(0, 3)
    spare = torch.zeros(3 * YS + 16, dtype=torch.uint8, device="cuda")
    assert a.add(0, 3, bufs=(pt, spare[8:], z), expect=INVALID) == INVALID and "d_y" in err()  # 8-byte aligned only: never launched
    for k in (1, 31):
        assert a.add(0, 1, k=k, expect=INVALID) == INVALID and "k must be" in err()
    flat = a.mult.view(torch.int32)
    assert a.add(0, 3, mult=flat[1:], expect=INVALID) == INVALID and "d_mult" in err()  # 4-byte aligned only
    assert a.add(0, 3, rep=a.rep[4:], expect=INVALID) == INVALID and "d_report" in err()
    group = pkg.Group([0])
    try:
        assert a.add(0, 3, h=group._h, expect=INVALID) == INVALID and "aesw_vacc_add_device" in err(group)
        assert a.vlib.aesw_vacc_prepare(group._h) == INVALID and "aesw_vacc_prepare" in err(group)
        with pytest.raises(pkg.AeswError) as e:
            group.multiplicity_accumulator(12, 2)
        assert e.value.status == pkg.api.ERR_INVALID_ARG
    finally:
        group.close()
    # over the capacity (K = 12, N = 2 holds 1 + 3 blocks): nothing is enqueued
    big = ctx.alloc_witness(8, vc.VALUES)
    big_pt = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
    for first, count in ((2, 3), (0, 5), (4, 1), (5, 0), (1 << 63, 1 << 63)):
        assert a.add(first, count, bufs=(big_pt, big.y, big.z), expect=CAPACITY) == CAPACITY and "aesw_vacc_add_device" in err() and "capacity" in err()
    assert a.add(4, 0, bufs=(big_pt, big.y, big.z)) == OK  # an empty run at the very end is one ...
    assert a.add(0, 0, key=None) == OK                     # ... and launches nothing, whatever else is missing
    torch.cuda.synchronize()
    arena.check()
    assert untouched(arena, a.mult, a.rep)
    # the accumulator of libaesw_acc.so still refuses VALUES, and the Python face reports a capacity
    with pytest.raises(pkg.AeswError) as e:
        ctx.multiplicity_accumulator(12, 2, vc.VALUES).reset().add(0, pkg.Witness(big.y, big.y, big.z, None, None), n_blocks=1)
    assert e.value.status == pkg.api.ERR_INVALID_ARG
    with pytest.raises(pkg.AeswError) as e:
        ctx.multiplicity_accumulator(12, 2).reset().add_values(3, big_pt, big, c.kw, n_blocks=2)
    assert e.value.status == pkg.api.ERR_CAPACITY


def test_the_plain_c_example_compares_values_with_packed(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_vacc"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_vacc.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_vacc", "-laesw_acc", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k, n_sets in ((14, 3), (13, 2)):
        out = subprocess.run([str(exe), str(k), str(n_sets)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        n = pkg.block_capacity(k, n_sets)
        sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
        lines = re.findall(r"set (\d+): range (\d+) xor (\d+) sbox (\d+) mul2 (\d+) mul3 (\d+)", out.stdout)
        assert len(lines) == n_sets
        for line in lines:
            s, *sums = [int(v) for v in line]
            assert sums == [int(sel[5 * s + i].sum()) for i in range(5)], line
        assert "%d blocks in 2 runs" % n in out.stdout and "%d lookups, 0 misses" % (400 + 1056 * n) in out.stdout, out.stdout
        assert "VALUES and PACKED agree in %d bins" % (n_sets * 66561) in out.stdout, out.stdout
