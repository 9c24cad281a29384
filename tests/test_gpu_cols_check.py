"""aesw_cols_check_device / Context.check_columns on the GPU: MockProver's criterion over the ASSEMBLED advice columns, bytes
and Fr cells, in one launch.  The case list is tests/cols_check_cases.py.

Expected reports come from the host model tests/cols_model.py (de-assemble with aesw_block_placement, the CPU run of
aesw_check.h, numpy for stray and non-canonical cells; tests/test_cols_model.py holds it against the oracle), never from the
kernel.  A single cell belongs to one circuit, so a corruption's expected report recomputes that circuit alone and takes the
others from the untouched run.  The report lies in a poisoned, guard-banded buffer (tests/guarded.py)."""
import numpy as np
import pytest

import cols_check_cases as ccs
import cols_model as cm
import guarded as G

pytestmark = pytest.mark.gpu

PT_FIELDS = ("lookup_failures", "copy_failures", "gate_failures", "input_failures", "first")
CELL_FIELDS = ("cell_failures", "unassigned_failures", "first_cell", "offset_failures", "satisfied")


@pytest.fixture(scope="module")
def lane(pkg):
    return cm.load_lane_model()


class Batch:
    """C circuits on the device, their slabs in `layout`, and their assembled columns in both forms."""

    def __init__(self, pkg, ctx, k, n_sets, counts, seed, layout=1, forms=(False, True)):
        import torch
        self.pkg, self.ctx, self.k, self.n_sets, self.layout = pkg, ctx, k, n_sets, layout
        self.counts = [int(c) for c in counts]
        self.nc, self.n = len(counts), int(sum(counts))
        self.offs = pkg.circuit_offsets(k, n_sets, counts, self.n)
        rng = np.random.default_rng(seed)
        self.keys = torch.from_numpy(rng.integers(0, 256, (self.nc, 16), dtype=np.uint8)).cuda()
        self.pt = torch.from_numpy(rng.integers(0, 256, (max(self.n, 0), 16), dtype=np.uint8)).cuda()
        self.adv = {}
        if layout == 1:  # the product path
            self.wit, self.kw, adv = ctx.circuits(k, n_sets, self.keys, self.pt, self.counts, as_fr=forms[0])
            self.adv[forms[0]] = adv
        else:
            self.kw = ctx.key_schedule_witness(self.keys, layout, want_rk=False)
            per_block = torch.repeat_interleave(self.keys, torch.as_tensor(self.counts, dtype=torch.int64, device="cuda"), dim=0)
            self.wit = ctx.encrypt_witness(self.pt, per_block, layout, want_ct=True) if self.n else ctx.alloc_witness(1, layout, want_ct=True)
        self.ct = self.wit.ct if self.n else None
        self.d_offs = torch.from_numpy(self.offs.view(np.int64)).cuda()
        for f in forms:
            if f not in self.adv:
                self.adv[f] = self.assemble(f)
        torch.cuda.synchronize()
        self.model = cm.ColsModel(cm.load_lane_model(), np.concatenate(ctx._tables), pkg, k, n_sets, self.offs)

    def assemble(self, as_fr):
        return self.ctx.assemble_advice_circuits(self.k, self.n_sets, self.wit, self.kw, self.counts, as_fr=as_fr, layout=self.layout,
                                                 n_blocks=self.n, _offsets=self.d_offs)

    def raw(self, report, as_fr, keys=True, ct=True, offsets=None, n=None):
        lib = self.pkg.api.load_cols_library()
        ctx, n = self.ctx, self.n if n is None else n
        rc = lib.aesw_cols_check_device(
            ctx._h, self.k, self.n_sets, self.nc, (self.d_offs if offsets is None else offsets).data_ptr(), n, self.pt.data_ptr() if n else None,
            self.keys.data_ptr() if keys else None, self.ct.data_ptr() if ct and self.ct is not None else None, 1 if as_fr else 0,
            self.adv[as_fr].data_ptr(), report.data_ptr(), ctx._stream())
        assert rc == 0, (rc, ctx._lib.aesw_last_error(ctx._h))

    def check(self, arena, as_fr, **kw):
        import torch
        rep = arena.out("report", 96)
        assert arena.poisoned(rep)
        self.raw(rep, as_fr, **kw)
        torch.cuda.synchronize()
        arena.check()
        return self.pkg.api.cols_report_dict(rep.view(torch.int64))

    # -- the expected side
    def host(self, keys=True, ct=True):
        return (self.pt.cpu().numpy(), self.keys.cpu().numpy() if keys else None,
                self.ct.cpu().numpy() if ct and self.ct is not None else None)

    def expect_circuit(self, c, as_fr, keys=True, ct=True):
        pt, ks, cts = self.host(keys, ct)
        return self.model.circuit(c, self.adv[as_fr][c].cpu().numpy(), pt, ks, cts)

    def clean(self):
        return {"blocks": self.n, "keys": self.nc, "lookup_failures": 0, "copy_failures": 0, "gate_failures": 0, "input_failures": 0,
                "first": None, "offset_failures": 0, "cell_failures": 0, "unassigned_failures": 0, "first_cell": None,
                "cells": self.nc * (3 * self.n_sets + 1) << self.k, "satisfied": True}


@pytest.mark.parametrize("layout", ccs.SLAB_LAYOUTS, ids=["dense", "packed"])
@pytest.mark.parametrize("k,n_sets,nc", ccs.SHAPES, ids=["k%d-n%d-c%d" % s for s in ccs.SHAPES])
def test_the_columns_of_context_circuits_are_satisfied(pkg, ctx, k, n_sets, nc, layout):
    import torch
    b = Batch(pkg, ctx, k, n_sets, ccs.counts(pkg, k, n_sets, nc), seed=k * 10 + nc, layout=layout)
    if k == 11:
        assert 0 in b.counts
    if k == 16:
        assert b.counts == [pkg.block_capacity(k, n_sets)] * nc
    arena = G.DeviceArena(G.CANARIES[(k + layout) % 2])
    for as_fr in ccs.FORMS:
        for keys, ct in ((True, True), (False, False)):
            assert b.check(arena, as_fr, keys=keys, ct=ct) == b.clean(), (as_fr, keys, ct)
        # the Python face
        assert ctx.check_columns(k, n_sets, b.pt, b.keys, b.adv[as_fr], b.counts, ct=b.ct) == b.clean()
        rep = ctx.check_columns(k, n_sets, b.pt, None, b.adv[as_fr], b.counts, sync=False, _offsets=b.d_offs)
        torch.cuda.synchronize()
        assert tuple(rep.shape) == (12,) and pkg.api.cols_report_dict(rep) == b.clean()
    # the model agrees on the smaller shapes (the expected side of the other tests)
    if k <= 12:
        pt, ks, cts = b.host()
        for as_fr in ccs.FORMS:
            assert b.model.check(b.adv[as_fr].cpu().numpy(), pt, ks, cts) == b.clean()
    with pytest.raises(ValueError):
        ctx.check_columns(k, n_sets, b.pt, b.keys, b.adv[False][:, :, :-1], b.counts)


def test_one_circuit_assemble_output_in_every_geometry_and_store_mode(pkg, ctx):
    import torch
    k, n_sets = 13, 2
    n = pkg.block_capacity(k, n_sets) - 1
    rng = np.random.default_rng(13)
    key = torch.from_numpy(rng.integers(0, 256, (1, 16), dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    geo0, st0 = ctx.get_option("assemble_geometry"), ctx.get_option("fr_store_mode")
    try:
        for layout in (0, 1):
            kw = ctx.key_schedule_witness(key, layout, want_rk=False)
            wit = ctx.encrypt_witness(pt, key[0].contiguous(), layout, want_ct=True)
            clean = {"blocks": n, "keys": 1, "lookup_failures": 0, "copy_failures": 0, "gate_failures": 0, "input_failures": 0, "first": None,
                     "offset_failures": 0, "cell_failures": 0, "unassigned_failures": 0, "first_cell": None, "cells": 7 << k, "satisfied": True}
            adv = ctx.assemble_advice(k, n_sets, wit, kw, n, layout=layout, as_fr=False)
            assert ctx.check_columns(k, n_sets, pt, key, adv, [n], ct=wit.ct) == clean
            for geo in range(5):
                for store in range(3):
                    ctx.set_option("assemble_geometry", geo)
                    ctx.set_option("fr_store_mode", store)
                    adv = ctx.assemble_advice(k, n_sets, wit, kw, n, layout=layout, as_fr=True)
                    assert tuple(adv.shape) == (7, 1 << k, 32)
                    assert ctx.check_columns(k, n_sets, pt, key, adv, [n], ct=wit.ct) == clean, (layout, geo, store)
    finally:
        ctx.set_option("assemble_geometry", geo0)
        ctx.set_option("fr_store_mode", st0)
    torch.cuda.synchronize()


def _cases(b, rng, as_fr):
    """300 (kind, target, index, value) single-cell corruptions over every kind of place."""
    m, k, ncol = b.model, b.k, 3 * b.n_sets + 1
    cases = []

    def cell(c, col, row):
        return m.cell_index(c, col, row)

    full = [c for c in range(b.nc) if b.counts[c] > 0]
    for _ in range(24):
        for col in range(3):  # slab x / y / z cells
            c = int(rng.choice(full))
            s, r = m.place[int(rng.integers(0, b.counts[c]))]
            cases.append(("slab", cell(c, 3 * s + col, r + int(rng.integers(0, cm.AES_ROWS)))))
        for col in range(3):  # key rows
            cases.append(("key", cell(int(rng.integers(0, b.nc)), col, int(rng.integers(0, cm.KEY_ROWS)))))
        cases.append(("words", cell(int(rng.integers(0, b.nc)), ncol - 1, int(rng.integers(0, cm.WORDS_ROWS)))))
        # stray cells: behind the last block of a set, words_column from row 96 on, the rows of a circuit without blocks
        c = int(rng.integers(0, b.nc))
        a = m.assigned(c)
        col = int(rng.integers(0, ncol - 1))
        free = np.flatnonzero(~a[col])
        cases.append(("stray", cell(c, col, int(rng.choice(free)))))
        cases.append(("stray", cell(c, ncol - 1, int(rng.integers(cm.WORDS_ROWS, 1 << k)))))
        s, r = m.place[0]
        inside = np.flatnonzero(~a[3 * s + 1, r:r + cm.AES_ROWS]) if b.counts[c] else free
        cases.append(("stray", cell(c, 3 * s + 1 if b.counts[c] else col, (r if b.counts[c] else 0) + int(rng.choice(inside)))))
    # a round-key cell every block of the fullest circuit copies from
    e = [e for e in b.pkg.block_copy_graph() if e["src_space"] == 1][40]
    cases.append(("key", cell(int(np.argmax(b.counts)), int(e["src_col"]), int(e["src_row"]))))
    out = [(kind, "cols", i, int(rng.integers(1, 256))) for kind, i in cases]
    for name, t in (("pt", b.pt), ("ct", b.ct), ("keys", b.keys)):
        out += [("lit", name, int(rng.integers(0, t.numel())), int(rng.integers(1, 256))) for _ in range(20)]
    if as_fr:  # up to a third: a non-canonical cell (one bit of its 32 bytes flipped)
        for j in range(0, len(out), 3):
            if out[j][1] == "cols":
                out[j] = ("noncanon",) + out[j][1:3] + (int(rng.integers(0, 256)),)
    assert len(out) >= 300 and sum(1 for o in out if o[0] == "noncanon") * 3 <= len(out) + 2
    return out


@pytest.mark.parametrize("as_fr", ccs.FORMS, ids=["bytes", "fr"])
def test_single_cell_corruptions_match_the_model(pkg, ctx, as_fr):
    """At least 300 seeded single-cell corruptions per form, compared in every field (non-canonical cells: the five fields
    the header leaves specified).  None is skipped."""
    k, n_sets = 13, 2
    cap = pkg.block_capacity(k, n_sets)
    counts = [cap, 0, 3, cap - 1, 1, 0, 7]
    b = Batch(pkg, ctx, k, n_sets, counts, seed=77, forms=(as_fr,))
    arena = G.DeviceArena(G.CANARIES[int(as_fr)])
    m, adv = b.model, b.adv[as_fr]
    base = [b.expect_circuit(c, as_fr) for c in range(b.nc)]
    assert m.compose(base) == b.clean() == b.check(arena, as_fr)
    lut = __import__("torch").from_numpy(m.lut).cuda()
    flat = adv.view(-1, 32) if as_fr else adv.view(-1)
    per_circuit = (3 * n_sets + 1) << k
    kinds, failing = set(), 0
    for kind, target, i, v in _cases(b, np.random.default_rng(300 + int(as_fr)), as_fr):
        t = flat if target == "cols" else getattr(b, target).view(-1)
        old = t[i].clone()
        if kind == "noncanon":
            t[i, v // 8] ^= 1 << (v % 8)
        elif target == "cols" and as_fr:
            cur = int(np.flatnonzero((m.lut == old.cpu().numpy()).all(axis=1))[0])
            t[i] = lut[cur ^ v]  # canonical, another byte
        else:
            t[i] ^= v
        try:
            if target == "cols":
                c = i // per_circuit
            elif target == "keys":
                c = i // 16
            else:
                c = int(np.searchsorted(b.offs, i // 16, side="right")) - 1
            per = list(base)
            per[c] = b.expect_circuit(c, as_fr)
            exp = m.compose(per)
            got = b.check(arena, as_fr)
        finally:
            t[i] = old
        fields = CELL_FIELDS if kind == "noncanon" else tuple(exp)
        assert {f: got[f] for f in fields} == {f: exp[f] for f in fields}, (kind, target, i, v, got, exp)
        assert got["blocks"] == b.n and got["keys"] == b.nc and got["cells"] == exp["cells"]
        kinds.add(kind)
        failing += not got["satisfied"]
        if kind == "stray":
            assert got["unassigned_failures"] == 1 and got["first_cell"] == i, (i, got)
        if kind == "noncanon":
            assert got["cell_failures"] == 1 and got["first_cell"] == i, (i, got)
        if kind == "lit":
            assert got["input_failures"] >= 1, (target, got)
    assert kinds == ({"slab", "key", "words", "stray", "lit"} | ({"noncanon"} if as_fr else set())) and failing >= 200, (kinds, failing)
    assert b.check(arena, as_fr) == b.clean()  # everything restored


@pytest.mark.parametrize("as_fr", ccs.FORMS, ids=["bytes", "fr"])
def test_a_slab_corruption_is_seen_alike_by_the_slab_and_the_column_checker(pkg, ctx, as_fr):
    k, n_sets = 13, 2
    cap = pkg.block_capacity(k, n_sets)
    b = Batch(pkg, ctx, k, n_sets, [cap, 0, 5, 2], seed=5, forms=(as_fr,))
    arena = G.DeviceArena(G.CANARIES[0])
    rng = np.random.default_rng(55)
    strides = [pkg.column_stride(1, i) for i in range(3)]
    targets = [b.wit.x, b.wit.y, b.wit.z, b.kw.kx, b.kw.ky, b.kw.kz, b.kw.w]
    differ = 0
    for j in range(28):
        t = targets[j % 7]
        i, v = int(rng.integers(0, t.numel())), int(rng.integers(1, 256))
        t[i] ^= v
        try:
            b.adv[as_fr] = b.assemble(as_fr)
            slab = ctx.check_circuits(k, n_sets, b.pt, b.keys, b.wit, b.kw, b.counts, layout=1, ct=b.ct)
            cols = b.check(arena, as_fr)
        finally:
            t[i] ^= v
        assert {f: cols[f] for f in PT_FIELDS} == {f: slab[f] for f in PT_FIELDS}, (j, i, v, cols, slab)
        assert cols["cell_failures"] == cols["unassigned_failures"] == 0 and cols["first_cell"] is None
        differ += not cols["satisfied"]
    assert differ >= 20, differ
    assert strides[0] == cm.AES_ROWS


def test_swapped_key_rows_fail_exactly_those_circuits_round_key_copies(pkg, ctx):
    import torch
    k, n_sets = 13, 2
    b = Batch(pkg, ctx, k, n_sets, [4, 3, 0, 6], seed=9, forms=(False,))
    arena = G.DeviceArena(G.CANARIES[1])
    adv = b.adv[False]
    base = [b.expect_circuit(c, False) for c in range(b.nc)]
    rows = slice(0, cm.KEY_ROWS)
    a, c = 0, 3
    tmp = adv[a, :3, rows].clone()
    adv[a, :3, rows] = adv[c, :3, rows]
    adv[c, :3, rows] = tmp
    wtmp = adv[a, -1, :cm.WORDS_ROWS].clone()
    adv[a, -1, :cm.WORDS_ROWS] = adv[c, -1, :cm.WORDS_ROWS]
    adv[c, -1, :cm.WORDS_ROWS] = wtmp
    torch.cuda.synchronize()
    got = b.check(arena, False)
    per = list(base)
    for i in (a, c):
        per[i] = b.expect_circuit(i, False)
    assert got == b.model.compose(per)
    # the key rows are a consistent schedule of the OTHER key: only the blocks' round-key copies and the key literals object
    assert got["lookup_failures"] == got["gate_failures"] == 0 and got["copy_failures"] > 0 and got["input_failures"] == 32
    assert got["unassigned_failures"] == 0 and base[1] == per[1] and base[2] == per[2]
    nokeys = b.check(arena, False, keys=False)
    assert nokeys["input_failures"] == 0 and nokeys["copy_failures"] == got["copy_failures"]
    assert nokeys["first"][0] == 0 and not nokeys["first"][1] and nokeys["first"][2] == 2  # block 0 of circuit 0, a copy


@pytest.mark.parametrize("as_fr", ccs.FORMS, ids=["bytes", "fr"])
def test_offsets_are_counted_as_the_header_says(pkg, ctx, as_fr):
    import torch
    k, n_sets = 14, 1
    counts = [3, 0, 10, 4, 0, 5]
    assert pkg.block_capacity(k, n_sets) == 10
    b = Batch(pkg, ctx, k, n_sets, counts, seed=8, forms=(as_fr,))
    arena = G.DeviceArena(G.CANARIES[int(as_fr)])
    offs = [int(v) for v in b.offs]

    def run(edit, **kw):
        o = list(offs)
        for i, v in edit.items():
            o[i] = v
        return b.check(arena, as_fr, offsets=torch.tensor(o, dtype=torch.int64, device="cuda"), **kw), o

    def spec(o, n):  # include/aesw_circ.h, word for word
        return sum(1 for c in range(len(o) - 1) if o[c + 1] < o[c] or o[c + 1] - o[c] > 10) + (o[0] != 0) + (o[-1] != n)

    for edit, what in (({5: 16}, "decreasing pair"), ({3: 14}, "count above the capacity"), ({0: 1}, "offsets[0] != 0"), ({6: 23}, "offsets[C] != n")):
        got, o = run(edit)
        assert spec(o, b.n) == 1 and got["offset_failures"] == 1, (what, got)
        assert got["blocks"] == b.n and got["keys"] == 6 and not got["satisfied"] and got["cells"] == 6 * 4 << k
    got, o = run({}, n=21)
    assert got["offset_failures"] == 1 and got["blocks"] == 21
    got, o = run({0: 2, 2: 1, 6: 40})
    assert got["offset_failures"] == spec(o, b.n) == 5, (got, o)
    rng = np.random.default_rng(88)
    for _ in range(40):
        o = [int(v) for v in rng.integers(0, 30, 7)]
        if rng.integers(0, 2):
            o.sort()
        got, o = run(dict(enumerate(o)))
        assert got["offset_failures"] == spec(o, b.n), (o, got)
        assert got["blocks"] == b.n and got["keys"] == 6 and got["cell_failures"] == 0
    assert b.check(arena, as_fr) == b.clean()


def test_graph_replays_and_three_streams(pkg, ctx):
    import torch
    k, n_sets = 13, 2
    b = Batch(pkg, ctx, k, n_sets, [6, 0, 7, 2], seed=14)
    b.adv[False][2, 4, 300] ^= 1
    b.adv[True][0, 6, 5000, 3] ^= 0x10  # words_column far behind row 96: non-canonical and never assigned
    torch.cuda.synchronize()
    arena = G.DeviceArena(G.CANARIES[0])
    for as_fr in ccs.FORMS:
        eager = b.check(arena, as_fr)
        assert eager == b.model.compose([b.expect_circuit(c, as_fr) for c in range(b.nc)]) and not eager["satisfied"]
        rep = arena.out("graph_report_%d" % as_fr, 96)
        torch.cuda.synchronize()
        cap = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            b.raw(rep, as_fr)
        torch.cuda.synchronize()
        assert arena.poisoned(rep), "the captured call ran during capture"
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert pkg.api.cols_report_dict(rep.view(torch.int64)) == eager
            rep.fill_(arena.canary)
        arena.check()
        streams = [torch.cuda.Stream() for _ in range(3)]
        reps = [arena.out("stream_report_%d_%d" % (as_fr, i), 96) for i in range(3)]
        torch.cuda.synchronize()
        for s, r in zip(streams, reps):
            with torch.cuda.stream(s):
                b.raw(r, as_fr)
        torch.cuda.synchronize()
        arena.check()
        for r in reps:
            assert pkg.api.cols_report_dict(r.view(torch.int64)) == eager


def test_argument_rules(pkg, ctx):
    import torch
    b = Batch(pkg, ctx, 12, 1, [1, 0, 1], seed=3, forms=(False,))
    lib = pkg.api.load_cols_library()
    rep = torch.zeros(12, dtype=torch.int64, device="cuda")

    def call(ctx_h=None, k=12, n_sets=1, nc=3, offs=None, as_fr=0, cols=None, report=None, pt=None):
        return lib.aesw_cols_check_device(
            ctx._h if ctx_h is None else ctx_h, k, n_sets, nc, b.d_offs.data_ptr() if offs is None else offs, b.n,
            b.pt.data_ptr() if pt is None else pt, b.keys.data_ptr(), b.ct.data_ptr(), as_fr, b.adv[False].data_ptr() if cols is None else cols,
            rep.data_ptr() if report is None else report, ctx._stream())

    assert call() == 0
    for kw in (dict(k=8), dict(k=31), dict(n_sets=0), dict(n_sets=1025), dict(nc=0), dict(offs=b.d_offs.data_ptr() + 4), dict(offs=0),
               dict(cols=b.adv[False].data_ptr() + 8), dict(cols=0), dict(report=rep.data_ptr() + 4), dict(report=0), dict(as_fr=2),
               dict(pt=0)):
        assert call(**kw) == 1, kw  # AESW_ERR_INVALID_ARG
    torch.cuda.synchronize()
    g = pkg.Group([0])
    try:
        assert call(ctx_h=g._h) == 1
        with pytest.raises(pkg.AeswError):
            g.check_columns()
    finally:
        g.close()
