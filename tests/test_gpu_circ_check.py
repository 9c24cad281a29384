"""aesw_circ_check_witness_device / Context.check_circuits on the GPU: MockProver's criterion over a many-circuit batch in one
launch.  The case list is tests/circ_check_cases.py (both instantiations of libaesw_circ.so's kernel, the shapes of the
many-circuit assemble sweep, ragged counts with empty circuits and one full circuit).

Expected reports are COMPOSED from code that has tests of its own: for every circuit with blocks the shared-key
Context.check_witness on freshly allocated copies of that circuit's slices and key slab; for a circuit without blocks the key
slab alone through the CPU run of aesw_check.h (tests/lane_model, as tests/test_check_model.py runs it).  Counts add up and
`first` is the minimum after shifting block units by offsets[c] (key slabs: unit c).  The report, the kernel's one output,
always lies in a poisoned, guard-banded buffer (tests/guarded.py) whose guards are checked."""
import ctypes as C

import numpy as np
import pytest

import circ_check_cases as ccc
import circuit_cases as cc
import guarded as G

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
COUNTS = ("lookup_failures", "copy_failures", "gate_failures", "input_failures")


@pytest.fixture(scope="module")
def model(pkg):
    import __graft_entry__ as ge
    L = C.CDLL(str(ge.build_lane_model()))
    L.lane_model_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 9
    return L


class Batch:
    """C circuits on the device: keys [C,16], pt [n,16], the blocks' witness under each block's circuit key, C key slabs."""

    def __init__(self, pkg, ctx, layout, k, n_sets, counts, seed):
        import torch
        self.pkg, self.ctx, self.layout, self.k, self.n_sets = pkg, ctx, layout, k, n_sets
        self.counts = [int(c) for c in counts]
        self.nc, self.n = len(counts), int(sum(counts))
        self.offs = pkg.circuit_offsets(k, n_sets, counts, self.n)
        rng = np.random.default_rng(seed)
        self.keys = torch.from_numpy(rng.integers(0, 256, (self.nc, 16), dtype=np.uint8)).cuda()
        self.pt = torch.from_numpy(rng.integers(0, 256, (self.n, 16), dtype=np.uint8)).cuda()
        if layout == ccc.PACKED:  # the product path: three launches of Context.circuits
            self.wit, self.kw, _adv = ctx.circuits(k, n_sets, self.keys, self.pt, self.counts, as_fr=False)
        else:
            self.kw = ctx.key_schedule_witness(self.keys, layout, want_rk=False)
            per_block = torch.repeat_interleave(self.keys, torch.as_tensor(self.counts, dtype=torch.int64, device="cuda"), dim=0)
            self.wit = ctx.encrypt_witness(self.pt, per_block, layout, want_ct=True) if self.n else ctx.alloc_witness(1, layout, want_ct=True)
        self.ct = self.wit.ct if self.n else None
        self.d_offs = torch.from_numpy(self.offs.view(np.int64)).cuda()
        self.strides = [pkg.column_stride(layout, i) for i in range(3)]
        self.kstrides = [96] + [pkg.key_column_stride(layout, i) for i in range(3)]  # w, kx, ky, kz
        torch.cuda.synchronize()

    def raw(self, report, keys=True, ct=True, offsets=None, n=None):
        """The C entry point, the report written into `report` (a guarded uint8[64] view) on torch's current stream."""
        lib = self.pkg.api.load_circ_library()
        ctx, n = self.ctx, self.n if n is None else n
        ks = self.pkg.api.KeySlab(*[t.data_ptr() for t in self.kw[:4]])
        d_offs = self.d_offs if offsets is None else offsets
        rc = lib.aesw_circ_check_witness_device(
            ctx._h, self.k, self.n_sets, self.nc, d_offs.data_ptr(), n, self.pt.data_ptr() if n else None,
            self.keys.data_ptr() if keys else None, self.layout, self.wit.x.data_ptr() if n else None,
            self.wit.y.data_ptr() if n else None, self.wit.z.data_ptr() if n else None,
            self.ct.data_ptr() if ct and self.ct is not None else None, C.byref(ks), report.data_ptr(), ctx._stream())
        assert rc == 0, (rc, ctx._lib.aesw_last_error(ctx._h))

    def check(self, arena, **kw):
        import torch
        rep = arena.out("report", 64)
        assert arena.poisoned(rep)
        self.raw(rep, **kw)
        torch.cuda.synchronize()
        arena.check()
        return self.pkg.api.circ_report_dict(rep.view(torch.int64))

    # -- the expected side
    def key_alone(self, model, c, slab, keys=True):
        """Key slab c through the CPU run of aesw_check.h's check_key: [lookup, copy, gate, input, raw `first` with unit c]."""
        tab = np.concatenate(self.ctx._tables)
        h = [t.cpu().numpy() for t in slab]
        key = self.keys[c].cpu().numpy() if keys else None
        rep, dummy = np.zeros(7, np.uint64), np.zeros(16, np.uint8)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert model.lane_model_check(p(tab), self.layout, p(dummy), p(key), 0, 0, p(dummy), p(dummy), p(dummy), None,
                                      p(h[0]), p(h[1]), p(h[2]), p(h[3]), p(rep)) == 0
        assert int(rep[0]) == 0 and int(rep[1]) == 1
        first = int(rep[6])
        if first != NONE:
            assert first >> 20 == 0 and (first >> 19) & 1
            first = (c << 20) | (first & 0xFFFFF)
        return [int(v) for v in rep[2:6]] + [first]

    def circuit_report(self, model, c, keys=True, ct=True):
        """[lookup, copy, gate, input, raw `first` shifted into the batch] of circuit c alone, from code with its own tests.
        The shared-key check numbers a circuit's key slab as unit 0, between its block 0 and its block 1, so its `first` names
        only one of the two kinds; in the batch the key slab is unit c and the blocks start at offsets[c].  Both minima are
        therefore taken apart before they are shifted: the key slab's from the CPU model, the blocks' from the shared-key check
        (block by block, in order, where the key slab's failure hides them)."""
        pkg, lo, hi = self.pkg, int(self.offs[c]), int(self.offs[c + 1])
        slab = [self.kw[i][c * s:(c + 1) * s].clone() for i, s in enumerate(self.kstrides)]
        kr = self.key_alone(model, c, slab, keys)
        if hi == lo:
            return kr

        def shared(b0, b1):
            w1 = pkg.Witness(*[self.wit[i][b0 * s:b1 * s].clone() for i, s in enumerate(self.strides)], None, None)
            r = self.ctx.check_witness(self.pt[b0:b1].clone(), self.keys[c].clone() if keys else None, w1, pkg.KeyWitness(*slab, None),
                                       layout=self.layout, ct=self.ct[b0:b1].clone() if ct and self.ct is not None else None)
            assert r["blocks"] == b1 - b0 and r["keys"] == 1
            return r

        r = shared(lo, hi)
        tot = [r[f] for f in COUNTS]
        blocks_first = NONE
        if r["first"] is not None and not r["first"][1]:
            unit, _is_key, kind, index = r["first"]
            blocks_first = ((lo + unit) << 20) | (kind << 16) | index
        elif tot != kr[:4]:  # the key slab's failure comes first in the circuit's own numbering: find the first failing block behind it
            assert r["first"][1] and (r["first"][2] << 16 | r["first"][3]) == kr[4] & 0x7FFFF
            for b in range(lo + 1, hi):
                f = shared(b, b + 1)["first"]
                if not f[1]:
                    blocks_first = (b << 20) | (f[2] << 16) | f[3]
                    break
            assert blocks_first != NONE
        if r["first"] is not None and r["first"][1]:
            assert (r["first"][2] << 16 | r["first"][3]) == kr[4] & 0x7FFFF  # device and CPU model name the same key-slab check
        assert all(t >= k_ for t, k_ in zip(tot, kr[:4]))
        return tot + [min(blocks_first, kr[4])]

    def compose(self, per_circuit):
        tot = [sum(r[i] for r in per_circuit) for i in range(4)]
        f = min(r[4] for r in per_circuit)
        first = None if f == NONE else (f >> 20, bool((f >> 19) & 1), (f >> 16) & 7, f & 0xFFFF)
        out = {"blocks": self.n, "keys": self.nc, "first": first, "offset_failures": 0, "satisfied": not any(tot)}
        out.update(dict(zip(COUNTS, tot)))
        return out


def _counts(pkg, k, n_sets, nc, seed):
    rows = 1 << k
    cap, cap0 = pkg.block_capacity(k, n_sets), (rows - 1760) // 1360 if rows >= 1760 else 0
    counts = cc.ragged_counts(cap, cap0, n_sets, nc, np.random.default_rng(seed))
    if nc > 2 and cap:
        assert counts[0] == cap and counts[1] == 0  # one full circuit, one empty one
    return counts


@pytest.mark.parametrize("layout", ccc.LAYOUTS, ids=["dense", "packed"])
@pytest.mark.parametrize("k,n_sets,nc", ccc.SHAPES, ids=["k%d-n%d-c%d" % s for s in ccc.SHAPES])
def test_a_batch_of_context_circuits_is_satisfied(pkg, ctx, k, n_sets, nc, layout):
    import torch
    b = Batch(pkg, ctx, layout, k, n_sets, _counts(pkg, k, n_sets, nc, k * 100 + n_sets * 10 + nc), seed=k + nc)
    arena = G.DeviceArena(G.CANARIES[(k + layout) % 2])
    clean = {"blocks": b.n, "keys": nc, "lookup_failures": 0, "copy_failures": 0, "gate_failures": 0, "input_failures": 0,
             "first": None, "offset_failures": 0, "satisfied": True}
    for keys in (True, False):
        for ct in (True, False):
            assert b.check(arena, keys=keys, ct=ct) == clean, (keys, ct)
    # the Python face: host-validated counts, and the report tensor of sync=False
    assert ctx.check_circuits(k, n_sets, b.pt, b.keys, b.wit, b.kw, b.counts, layout=layout, ct=b.ct) == clean
    assert ctx.check_circuits(k, n_sets, b.pt, None, b.wit, b.kw, b.counts, layout=layout) == clean
    rep = ctx.check_circuits(k, n_sets, b.pt, b.keys, b.wit, b.kw, b.counts, layout=layout, ct=b.ct, sync=False, _offsets=b.d_offs)
    torch.cuda.synchronize()
    assert tuple(rep.shape) == (8,) and pkg.api.circ_report_dict(rep) == clean
    with pytest.raises(ValueError):
        ctx.check_circuits(k, n_sets, b.pt, b.keys, b.wit, b.kw, b.counts + [1], layout=layout)


def _round_key_cell(pkg, layout):
    """(name of the key slab column, index in it) of a key cell an AddRoundKey row of every block copies from."""
    e = [e for e in pkg.block_copy_graph() if e["src_space"] == 1][40]  # space 1: the key slab (aesw_check.h build_check_table)
    col, row = int(e["src_col"]), int(e["src_row"])
    idx = row if layout == ccc.DENSE else int(pkg.key_packed_index(col)[row])
    assert idx >= 0
    return ("kx", "ky", "kz")[col], idx


@pytest.mark.parametrize("layout", ccc.LAYOUTS, ids=["dense", "packed"])
def test_single_byte_corruptions_compose(pkg, ctx, model, layout):
    """300 seeded single-byte corruptions -- 30 each in x, y, z, kx, ky, kz, words, pt, ct, keys -- plus a round-key cell of the
    full circuit (142 blocks copy from it), corruptions of an empty circuit's key slab and key, and the untouched batch: the
    one-launch report equals the composed one in every field.  None is skipped.  A single byte belongs to one circuit, so the
    composition takes the other circuits' reports from the untouched run (their inputs are byte for byte the same)."""
    import torch
    k, n_sets, nc = 16, 3, 37
    counts = _counts(pkg, k, n_sets, nc, 7)
    b = Batch(pkg, ctx, layout, k, n_sets, counts, seed=31 + layout)
    assert counts[0] == 142 and counts[1] == 0
    arena = G.DeviceArena(G.CANARIES[layout])
    base = [b.circuit_report(model, c) for c in range(nc)]
    assert all(r == [0, 0, 0, 0, NONE] for r in base)
    assert b.check(arena) == b.compose(base)

    targets = {"x": b.wit.x, "y": b.wit.y, "z": b.wit.z, "kx": b.kw.kx, "ky": b.kw.ky, "kz": b.kw.kz, "w": b.kw.w,
               "pt": b.pt.view(-1), "ct": b.ct.view(-1), "keys": b.keys.view(-1)}
    per_unit = {"x": b.strides[0], "y": b.strides[1], "z": b.strides[2], "kx": b.kstrides[1], "ky": b.kstrides[2], "kz": b.kstrides[3],
                "w": 96, "pt": 16, "ct": 16, "keys": 16}
    rng = np.random.default_rng(300 + layout)
    cases = [(name, int(rng.integers(0, targets[name].numel())), int(rng.integers(1, 256))) for name in targets for _ in range(30)]
    rk_col, rk_idx = _round_key_cell(pkg, layout)
    cases.append((rk_col, rk_idx, 0x40))  # key slab 0: the full circuit's
    cases += [("kx", 1 * per_unit["kx"] + 5, 1), ("w", 1 * 96 + 3, 0x80), ("w", 1 * 96 + 40, 2), ("keys", 16 + 9, 0x10)]  # circuit 1: no block
    assert len(cases) >= 300
    seen, failing = set(), 0
    for name, i, v in cases:
        t = targets[name]
        unit = i // per_unit[name]
        c = unit if name in ("kx", "ky", "kz", "w", "keys") else int(np.searchsorted(b.offs, unit, side="right")) - 1
        t[i] ^= v
        try:
            per = list(base)
            per[c] = b.circuit_report(model, c)
            exp = b.compose(per)
            got = b.check(arena)
        finally:
            t[i] ^= v
        assert got == exp, (name, i, v, c, got, exp)
        seen.add(name)
        failing += not got["satisfied"]
        if (name, i, v) == (rk_col, rk_idx, 0x40):
            assert got["copy_failures"] >= 142 and got["first"][0] == 0, got  # every block of the full circuit notices
        if name in ("pt", "ct", "keys"):
            assert got["input_failures"] >= 1, (name, got)
    assert seen == set(targets) and failing >= 90, (sorted(seen), failing)  # the 90 literal bytes at least (DENSE holds never-assigned cells)
    assert b.check(arena) == b.compose(base)  # everything restored


@pytest.mark.parametrize("layout", ccc.LAYOUTS, ids=["dense", "packed"])
def test_offsets_are_walked_and_reported(pkg, ctx, layout):
    """A block moved across a circuit boundary (the device offsets edited, passed unvalidated) fails exactly its round-key
    copies; every kind of broken offset list is counted exactly.  Nothing here reads outside the buffers: the circuit comes
    from the search tests/test_circ_search.py holds inside [0, C) for any offsets, every block index stays below n."""
    import torch
    k, n_sets = 14, 1
    counts = [3, 0, 10, 4, 0, 5]
    assert pkg.block_capacity(k, n_sets) == 10
    b = Batch(pkg, ctx, layout, k, n_sets, counts, seed=8)
    arena = G.DeviceArena(G.CANARIES[1 - layout])
    offs = [int(v) for v in b.offs]
    assert offs == [0, 3, 3, 13, 17, 17, 22]

    def run(edit, **kw):
        o = list(offs)
        for i, v in edit.items():
            o[i] = v
        return b.check(arena, offsets=torch.tensor(o, dtype=torch.int64, device="cuda"), **kw), o

    def spec(o, n):  # include/aesw_circ.h, word for word
        return sum(1 for c in range(len(o) - 1) if o[c + 1] < o[c] or o[c + 1] - o[c] > 10) + (o[0] != 0) + (o[-1] != n)

    # block 17, the first of circuit 5, handed to circuit 3 (circuit 4 stays empty): still valid offsets
    got, o = run({4: 18, 5: 18})
    assert spec(o, b.n) == 0 and got["offset_failures"] == 0
    lone = pkg.Witness(*[b.wit[i][17 * s:18 * s].clone() for i, s in enumerate(b.strides)], None, None)
    slab3 = pkg.KeyWitness(*[b.kw[i][3 * s:4 * s].clone() for i, s in enumerate(b.kstrides)], None)
    alone = ctx.check_witness(b.pt[17:18].clone(), b.keys[3].clone(), lone, slab3, layout=layout, ct=b.ct[17:18].clone())
    assert alone["copy_failures"] > 0 and alone["lookup_failures"] == alone["input_failures"] == alone["gate_failures"] == 0
    assert alone["first"][0] == 0 and not alone["first"][1] and alone["first"][2] == 2
    assert {f: got[f] for f in COUNTS} == {f: alone[f] for f in COUNTS}, (got, alone)  # that block's round-key copies, nothing else
    assert got["first"] == (17,) + tuple(alone["first"][1:]) and got["blocks"] == 22 and got["keys"] == 6

    # each kind of broken list on its own: exactly one failure each
    for edit, what in (({5: 16}, "decreasing pair"), ({3: 14}, "count above the capacity"), ({0: 1}, "offsets[0] != 0"), ({6: 23}, "offsets[C] != n")):
        got, o = run(edit)
        assert spec(o, b.n) == 1 and got["offset_failures"] == 1, (what, got)
        assert got["blocks"] == b.n and got["keys"] == 6 and not got["satisfied"]
    # n as the call was told decides the last one
    got, o = run({}, n=21)
    assert got["offset_failures"] == 1 and got["blocks"] == 21
    # several at once, and seeded lists of every kind
    got, o = run({0: 2, 2: 1, 6: 40})
    assert got["offset_failures"] == spec(o, b.n) == 5, (got, o)
    rng = np.random.default_rng(88)
    for _ in range(40):
        o = [int(v) for v in rng.integers(0, 30, 7)]
        if rng.integers(0, 2):
            o.sort()
        got, o = run(dict(enumerate(o)))
        assert got["offset_failures"] == spec(o, b.n), (o, got)
        assert got["blocks"] == b.n and got["keys"] == 6
    assert b.check(arena)["satisfied"]


def test_graph_replays_and_three_streams(pkg, ctx, model):
    """Captured into a hipGraph and replayed three times into the same (re-poisoned) report: the eager report each time.  Then
    the same context on three streams at once: three equal reports."""
    import torch
    k, n_sets = 14, 3
    counts = [34, 0, 7, 34, 11]
    b = Batch(pkg, ctx, ccc.PACKED, k, n_sets, counts, seed=14)
    b.wit.z[50 * b.strides[2] + 100] ^= 1   # block 50, circuit 3
    b.kw.w[2 * 96 + 1] ^= 4                 # key slab 2
    torch.cuda.synchronize()
    arena = G.DeviceArena(G.CANARIES[0])
    eager = b.check(arena)
    assert eager == b.compose([b.circuit_report(model, c) for c in range(len(counts))])
    assert not eager["satisfied"] and eager["first"][0] == 2 and eager["first"][1]

    rep = arena.out("graph_report", 64)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        b.raw(rep)
    torch.cuda.synchronize()
    assert arena.poisoned(rep), "the captured call ran during capture"
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert pkg.api.circ_report_dict(rep.view(torch.int64)) == eager
        rep.fill_(arena.canary)
    arena.check()

    streams = [torch.cuda.Stream() for _ in range(3)]
    reps = [arena.out("stream_report_%d" % i, 64) for i in range(3)]
    torch.cuda.synchronize()
    for s, r in zip(streams, reps):
        with torch.cuda.stream(s):
            b.raw(r)
    torch.cuda.synchronize()
    arena.check()
    for r in reps:
        assert pkg.api.circ_report_dict(r.view(torch.int64)) == eager


def test_argument_rules(pkg, ctx):
    import torch
    b = Batch(pkg, ctx, ccc.PACKED, 14, 1, [2, 0, 1], seed=3)
    lib = pkg.api.load_circ_library()
    rep = torch.zeros(8, dtype=torch.int64, device="cuda")
    ks = pkg.api.KeySlab(*[t.data_ptr() for t in b.kw[:4]])

    def call(ctx_h=None, k=14, n_sets=1, nc=3, offs=None, layout=ccc.PACKED, x=None, slab=ks, report=None):
        return lib.aesw_circ_check_witness_device(
            ctx._h if ctx_h is None else ctx_h, k, n_sets, nc, b.d_offs.data_ptr() if offs is None else offs, b.n, b.pt.data_ptr(),
            b.keys.data_ptr(), layout, b.wit.x.data_ptr() if x is None else x, b.wit.y.data_ptr(), b.wit.z.data_ptr(), b.ct.data_ptr(),
            C.byref(slab) if slab is not None else None, rep.data_ptr() if report is None else report, ctx._stream())

    assert call() == 0
    bad_slab = pkg.api.KeySlab(b.kw.w.data_ptr(), b.kw.kx.data_ptr(), b.kw.ky.data_ptr(), b.kw.kz.data_ptr() + 8)
    for kw in (dict(layout=2), dict(k=1), dict(k=31), dict(n_sets=0), dict(n_sets=1025), dict(nc=0), dict(offs=b.d_offs.data_ptr() + 4),
               dict(x=b.wit.x.data_ptr() + 4), dict(slab=None), dict(slab=bad_slab), dict(report=rep.data_ptr() + 4)):
        assert call(**kw) == 1, kw  # AESW_ERR_INVALID_ARG
    torch.cuda.synchronize()
    g = pkg.Group([0])
    try:
        assert call(ctx_h=g._h) == 1
        with pytest.raises(pkg.AeswError):
            g.check_circuits()
    finally:
        g.close()
