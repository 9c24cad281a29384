"""aesw_theta_inputs_device / Context.lookup_inputs on the GPU: the compressed input column of every argument in row order, as
table-row indices (tests/theta_cases.py: tc.INPUT_SHAPES).  Expected values come from tests/theta_model.py alone, over the advice
matrix and the selector columns of the circuit -- the oracle's own synthesize() from k = 11 on; below that, where 2^k rows do
not hold a circuit the oracle builds, zeros with the DENSE key slab at the key rows and the selectors of
aesw_assemble_selectors.  d_in and the report lie in poisoned, guard-banded buffers (tests/guarded.py)."""
import ctypes as C

import numpy as np
import pytest

import guarded as G
import theta_cases as tc
import theta_model as tm

pytestmark = pytest.mark.gpu
OK, INVALID, CAPACITY = 0, 1, 5
DENSE, PACKED, VALUES = 0, 1, 2
AES_ROWS, KEY_ROWS = 1360, 400
ORACLE_MAX_SETS = 64  # oracle/aesw_oracle.c: MAX_SETS


class World:
    """One circuit: its slabs on the device in both layouts, and what the prover holds of it on the host."""

    def __init__(self, pkg, ctx, oracle, k, n_sets, n, identical=False):
        import torch
        self.pkg, self.ctx, self.k, self.n_sets, self.n = pkg, ctx, k, n_sets, n
        rng = np.random.default_rng(1000 * k + 10 * n_sets + n)
        key, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
        if identical:
            pt[:] = pt[0]
        d_key, d_pt = torch.from_numpy(key).cuda(), torch.from_numpy(pt).cuda()
        empty = lambda: torch.empty(0, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.w = {l: ctx.encrypt_witness(d_pt, d_key, l) if n else pkg.Witness(empty(), empty(), empty(), None, None) for l in (DENSE, PACKED)}
        self.kw = {l: ctx.key_schedule_witness(d_key.reshape(1, 16), l, want_rk=False) for l in (DENSE, PACKED)}
        torch.cuda.synchronize()
        if k >= 11 and n_sets > ORACLE_MAX_SETS:
            self.advice, self.sel = self.from_slabs(oracle, key, pt), pkg.assemble_selectors(k, n_sets, n)[0]
        elif k >= 11:
            with oracle.circuit(k, n_sets, key, pt, record_copies=False) as c:
                assert c.status == 0
                self.advice = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
                self.sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
        else:
            assert n == 0
            self.advice = np.zeros((3 * n_sets + 1, 1 << k), np.uint8)
            if k >= 9:
                for c in range(3):
                    self.advice[c, :KEY_ROWS] = self.kw[DENSE][1 + c].cpu().numpy()
            self.sel = pkg.assemble_selectors(k, n_sets, 0)[0]
        self.tables = oracle.tables()

    def from_slabs(self, oracle, key, pt):
        """The advice matrix without the oracle's circuit (which holds at most ORACLE_MAX_SETS sets): the oracle's DENSE slabs, the
        key slab at the key rows and block b at block_placement(b).  The model reads no cell of the words column."""
        k, n_sets, n = self.k, self.n_sets, self.n
        advice = np.zeros((3 * n_sets + 1, 1 << k), np.uint8)
        w, kw = oracle.encrypt_witness(pt, key, layout=DENSE), oracle.key_schedule_witness(key, layout=DENSE)
        for c, name in enumerate(("kx", "ky", "kz")):
            advice[c, :KEY_ROWS] = getattr(kw, name)[:KEY_ROWS]
        for b in range(n):
            st, first = self.pkg.block_placement(k, n_sets, b)
            for c, name in enumerate("xyz"):
                advice[3 * st + c, first:first + AES_ROWS] = getattr(w, name)[b * AES_ROWS:(b + 1) * AES_ROWS]
        return advice

    def expected(self, keyed=True, advice=None):
        sel = self.sel.copy()
        if not keyed:
            sel[:5, :KEY_ROWS] = 0
        return tm.input_columns(self.advice if advice is None else advice, sel, self.tables)


class Call:
    """The C ABI on torch's current stream over a guarded d_in and report."""

    def __init__(self, w: World, arena):
        import torch
        self.torch, self.w, self.arena, self.lib = torch, w, arena, w.pkg.api.load_theta_library()
        self.out, self.rep = arena.out("in", (w.n_sets * 5 * 4) << w.k), arena.out("report", 24)

    def run(self, layout=PACKED, keyed=True, n=None, expect=OK, slabs=None, kw=None, h=None, k=None, n_sets=None, out=0, rep=0, prepare=True):
        w = self.w
        n = w.n if n is None else n
        slabs = w.w[layout if layout in (DENSE, PACKED) else PACKED][:3] if slabs is None else slabs
        kw = w.kw[layout if layout in (DENSE, PACKED) else PACKED] if kw is None else kw
        ks = w.pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]]) if keyed else None
        k, n_sets = w.k if k is None else k, w.n_sets if n_sets is None else n_sets
        if prepare and expect == OK:
            assert self.lib.aesw_theta_prepare(w.ctx._h, k, n_sets, w.ctx._stream()) == OK
        arg = lambda given, t: t.data_ptr() if given == 0 else given  # noqa: E731
        rc = self.lib.aesw_theta_inputs_device(w.ctx._h if h is None else h, k, n_sets, n, layout, *[t.data_ptr() if t.numel() else None for t in slabs],
                                               C.byref(ks) if ks is not None else None, arg(out, self.out), arg(rep, self.rep), w.ctx._stream())
        assert rc == expect, (rc, w.ctx._lib.aesw_last_error(w.ctx._h))

    def result(self):
        self.torch.cuda.synchronize()
        self.arena.check()
        col = self.out.view(self.torch.int32).cpu().numpy().view(np.uint32).reshape(self.w.n_sets, 5, 1 << self.w.k)
        return col.astype(np.int64), self.w.pkg.api.mult_report_dict(self.rep.view(self.torch.int64))

    def untouched(self):
        self.torch.cuda.synchronize()
        return self.arena.poisoned_on_device(self.out) and self.arena.poisoned_on_device(self.rep)


def same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert not bad.size, "%r: %d cells differ, first (set, tag - 1, row) %r: got %d, expected %d" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


_worlds = {}


def world(pkg, ctx, oracle, k, n_sets, n, identical=False):
    at = (k, n_sets, n, identical)
    if at not in _worlds:
        _worlds[at] = World(pkg, ctx, oracle, k, n_sets, n, identical)
    return _worlds[at]


def fills():
    """(k, n_sets, which) -> the block count is taken from aesw_block_capacity when the test runs"""
    return [(k, n_sets, which) for k, n_sets in tc.INPUT_SHAPES for which in (("full",) if k < 11 else ("part", "full"))]


@pytest.mark.parametrize("k,n_sets,which", fills())
def test_every_cell_of_every_argument(pkg, ctx, oracle, k, n_sets, which):
    cap = pkg.block_capacity(k, n_sets)
    assert (cap == 0) == (k < 11)
    n = cap if which == "full" else cap // 2
    w = world(pkg, ctx, oracle, k, n_sets, n)
    for i, (layout, keyed) in enumerate(((PACKED, True), (DENSE, True), (PACKED, False), (DENSE, False))):
        c = Call(w, G.DeviceArena(G.CANARIES[i % 2]))
        assert c.untouched()
        c.run(layout, keyed)
        got, rep = c.result()
        exp, lookups, misses = w.expected(keyed)
        same(got, exp, (k, n_sets, n, layout, keyed))
        assert misses == 0 and rep == {"lookups": lookups, "misses": 0, "first_miss": None}
        assert lookups == 1056 * n + (400 if keyed and k >= 9 else 0)
        if k < 9:
            assert (got == tm.ZERO_ROW).all()
        if not n:
            continue
        # the same slabs through the multiplicity library: every column's bincount is its section
        mult, mrep = ctx.lookup_multiplicities(k, n_sets, pkg.Witness(*w.w[layout][:3], None, None), w.kw[layout] if keyed else None, [n], layout)
        hist = mult.cpu().numpy().view(np.uint32)[0]
        assert mrep == rep
        for s in range(n_sets):
            for tag, (first, rows) in zip((1, 2, 3, 4, 5), tm.SECTIONS):
                counts = np.bincount(got[s, tag - 1], minlength=tm.BINS)
                assert np.array_equal(counts[first:first + rows], hist[s, first:first + rows]) and counts[tm.ZERO_ROW] == (1 << k) - hist[s, first:first + rows].sum()


@pytest.mark.parametrize("k,n_sets", [s for s in tc.INPUT_SHAPES if s[0] >= 11])
def test_one_more_block_than_the_circuit_holds_is_refused(pkg, ctx, oracle, k, n_sets):
    cap = pkg.block_capacity(k, n_sets)
    w = world(pkg, ctx, oracle, k, n_sets, cap)
    c = Call(w, G.DeviceArena())
    for layout in (PACKED, DENSE):
        c.run(layout, n=cap + 1, expect=CAPACITY)
        assert "aesw_theta_inputs_device" in ctx._lib.aesw_last_error(ctx._h).decode()
    c.arena.check()
    assert c.untouched()
    with pytest.raises(pkg.AeswError) as e:
        import torch
        twice = [torch.cat([t, t]) for t in w.w[PACKED][:3]]  # room for cap + 1 blocks: the library refuses, not the wrapper
        ctx.lookup_inputs(k, n_sets, pkg.Witness(*twice, None, None), w.kw[PACKED], n_blocks=cap + 1)
    assert e.value.status == pkg.api.ERR_CAPACITY


@pytest.mark.parametrize("layout", (PACKED, DENSE))
def test_planted_misses_mark_their_cell_and_nothing_else(pkg, ctx, oracle, layout):
    """y of an S-box row, z of an xor row of the last block, z of an xor row of the key slab: one at a time, then all three."""
    k, n_sets = 12, 3
    n = pkg.block_capacity(k, n_sets)
    w = world(pkg, ctx, oracle, k, n_sets, n)
    clean, lookups, _ = w.expected()
    index = (lambda col, r: r) if layout == DENSE else (lambda col, r: int(oracle.packed_index(col)[r]))
    kindex = (lambda col, r: r) if layout == DENSE else (lambda col, r: int(oracle.key_packed_index(col)[r]))
    stride = [pkg.column_stride(layout, c) for c in range(3)]
    plants = {"sbox": (1, 2, 32, 3), "xor": (2, n - 1, 1344, 2), "key": (2, None, 45, 2)}  # column, block (None: the key slab), slab row, tag
    for case in (("sbox",), ("xor",), ("key",), ("sbox", "xor", "key")):
        slabs, kw, advice = [t.clone() for t in w.w[layout][:3]], [t.clone() if t is not None else None for t in w.kw[layout]], w.advice.copy()
        cells, keys = [], []
        for name in case:
            col, block, r, tag = plants[name]
            if block is None:
                kw[1 + col][kindex(col, r)] ^= 0x21
                st, row = 0, r
                keys.append(0 << 20 | 1 << 19 | 1 << 16 | r)
            else:
                slabs[col][block * stride[col] + index(col, r)] ^= 0x21
                st, first = pkg.block_placement(k, n_sets, block)
                row = first + r
                keys.append(block << 20 | 1 << 16 | r)
            advice[3 * st + col, row] ^= 0x21
            cells.append((st, tag - 1, row))
        c = Call(w, G.DeviceArena(G.CANARIES[len(case) % 2]))
        c.run(layout, slabs=slabs, kw=kw)
        got, rep = c.result()
        exp, _, misses = w.expected(advice=advice)
        same(got, exp, (layout, case))
        assert misses == len(case) and sorted(map(tuple, np.argwhere(got != clean))) == sorted(cells), case
        assert all(got[at] == tm.MISS for at in cells)
        first = min(keys)
        assert rep == {"lookups": lookups, "misses": len(case), "first_miss": (first >> 20, bool(first >> 19 & 1), first & 0xFFFF)}, rep


def test_a_report_folded_from_more_parts_than_its_workgroup_has_threads(pkg, ctx, oracle):
    """k = 14 with 65 sets: 16 workgroups x 65 sets = 1 040 parts, so the 1 024 threads of theta_report_kernel walk the parts in two
    turns.  Blocks fill the sets in order, so a block of the last set needs every set in front of it full: all 778 blocks.  One
    miss in the last block, whose set's parts have indices 1 024 ... 1 039: the report's misses and first_miss arrive through
    one of them.  The oracle builds no circuit of 65 sets; the advice comes from its slabs (World.from_slabs), which is held
    against its circuit where it builds one."""
    small = world(pkg, ctx, oracle, 12, 3, pkg.block_capacity(12, 3))
    rng = np.random.default_rng(1000 * 12 + 10 * 3 + small.n)  # World's own key and plaintexts
    key, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (small.n, 16), dtype=np.uint8)
    assert np.array_equal(small.from_slabs(oracle, key, pt)[:9], small.advice[:9])
    assert np.array_equal(pkg.assemble_selectors(12, 3, small.n)[0], small.sel)

    k, n_sets = 14, 65
    n = pkg.block_capacity(k, n_sets)
    assert n == 778 and -(-(1 << k) // 1024) * n_sets == 1040
    w = world(pkg, ctx, oracle, k, n_sets, n)
    clean, lookups, none = w.expected()
    assert none == 0 and lookups == 1056 * n + 400
    st, first = pkg.block_placement(k, n_sets, n - 1)
    assert st == n_sets - 1 and st * 16 >= 1024
    r = 1344  # an xor row: z
    for layout in (PACKED, DENSE):
        at = r if layout == DENSE else int(oracle.packed_index(2)[r])
        slabs, advice = [t.clone() for t in w.w[layout][:3]], w.advice.copy()
        slabs[2][(n - 1) * pkg.column_stride(layout, 2) + at] ^= 0x21
        advice[3 * st + 2, first + r] ^= 0x21
        c = Call(w, G.DeviceArena(G.CANARIES[layout]))
        c.run(layout, slabs=slabs)
        got, rep = c.result()
        exp, _, misses = w.expected(advice=advice)
        same(got, exp, (k, n_sets, layout))
        assert misses == 1 and [tuple(x) for x in np.argwhere(got != clean)] == [(st, 1, first + r)] and got[st, 1, first + r] == tm.MISS
        assert rep == {"lookups": lookups, "misses": 1, "first_miss": (n - 1, False, r)}, rep


def test_identical_blocks(pkg, ctx, oracle):
    k, n_sets = 12, 3
    n = pkg.block_capacity(k, n_sets)
    w = world(pkg, ctx, oracle, k, n_sets, n, identical=True)
    c = Call(w, G.DeviceArena())
    c.run(PACKED)
    got, rep = c.result()
    exp, lookups, _ = w.expected()
    same(got, exp, "identical")
    assert rep["lookups"] == lookups and rep["misses"] == 0
    st, first = pkg.block_placement(k, n_sets, n - 1)
    s0, f0 = pkg.block_placement(k, n_sets, 1)
    assert np.array_equal(got[st, :, first:first + AES_ROWS], got[s0, :, f0:f0 + AES_ROWS])


def test_a_captured_call_rebuilds_column_and_report_on_every_replay(pkg, ctx, oracle):
    import torch
    k, n_sets = 12, 3
    n = pkg.block_capacity(k, n_sets)
    w = world(pkg, ctx, oracle, k, n_sets, n)
    slabs = [t.clone() for t in w.w[PACKED][:3]]
    slabs[2][3] ^= 0x10  # one miss: a report that accumulated would count it once per replay
    arena = G.DeviceArena()
    c = Call(w, arena)
    side = torch.cuda.Stream()
    handle = C.c_void_p(side.cuda_stream)
    # a capturing call cannot allocate: without a workspace for this context and stream it refuses, enqueues nothing and says how
    fresh = pkg.Context(0)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = c.lib.aesw_theta_inputs_device(fresh._h, k, n_sets, n, PACKED, *[t.data_ptr() for t in slabs], None, c.out.data_ptr(), c.rep.data_ptr(), handle)
            said = fresh._lib.aesw_last_error(fresh._h).decode()
        assert rc == INVALID and "aesw_theta_inputs_device" in said and "aesw_theta_prepare" in said, (rc, said)
        torch.cuda.synchronize()
        assert c.untouched()
    finally:
        fresh.close()
    assert c.lib.aesw_theta_prepare(ctx._h, k, n_sets, handle) == OK
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c.run(PACKED, slabs=slabs, prepare=False)
    torch.cuda.synchronize()
    assert c.untouched(), "the captured call ran during capture"
    first = None
    for i in range(3):
        graph.replay()
        got, rep = c.result()
        assert rep["misses"] == 1 and rep["lookups"] == 400 + 1056 * n and int((got == tm.MISS).sum()) == 1, (i, rep)
        first = got if first is None else first
        assert np.array_equal(got, first)
        arena.repoison()
        assert c.untouched()
        if i == 0:
            # a larger circuit on the same context and stream between two replays: the workspace grows next to the block the
            # graph holds, which is neither freed nor moved
            assert c.lib.aesw_theta_prepare(ctx._h, 20, 4, handle) == OK
            big = world(pkg, ctx, oracle, 11, 2, 0)
            with torch.cuda.stream(side):
                index, brep = ctx.lookup_inputs(13, 5, big.w[PACKED], big.kw[PACKED], n_blocks=0)
            assert brep == {"lookups": 400, "misses": 0, "first_miss": None} and tuple(index.shape) == (5, 5, 1 << 13)


def test_the_python_face(pkg, ctx, oracle):
    k, n_sets = 12, 3
    n = pkg.block_capacity(k, n_sets) // 2
    w = world(pkg, ctx, oracle, k, n_sets, n)
    index, rep = ctx.lookup_inputs(k, n_sets, pkg.Witness(*w.w[DENSE][:3], None, None), w.kw[DENSE], layout=DENSE)
    exp, lookups, _ = w.expected()
    assert tuple(index.shape) == (n_sets, 5, 1 << k) and rep == {"lookups": lookups, "misses": 0, "first_miss": None}
    same(index.cpu().numpy().view(np.uint32).astype(np.int64), exp, "python")


def test_refusals_leave_the_outputs_alone_and_say_why(pkg, ctx, oracle):
    k, n_sets = 12, 3
    w = world(pkg, ctx, oracle, k, n_sets, pkg.block_capacity(k, n_sets))
    c = Call(w, G.DeviceArena())
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    for kw, word in ((dict(layout=VALUES), "layout"), (dict(layout=7), "layout"), (dict(k=1), "k must be"), (dict(k=31), "k must be"), (dict(n_sets=0), "n_sets"),
                     (dict(n_sets=1025), "n_sets"), (dict(out=None), "d_in"), (dict(out=c.out.data_ptr() + 4), "d_in"), (dict(rep=None), "d_report"),
                     (dict(rep=c.rep.data_ptr() + 4), "d_report"), (dict(slabs=[t[1:] for t in w.w[PACKED][:3]]), "d_x"),
                     (dict(kw=[None] + [t[1:] for t in w.kw[PACKED][1:4]]), "key columns")):
        if "kw" in kw:
            kw["kw"][0] = w.kw[PACKED][0]
        c.run(expect=INVALID, **kw)
        assert "aesw_theta_inputs_device" in err() and word in err(), (kw, err())
    empty = [t[:0] for t in w.w[PACKED][:3]]
    c.run(expect=INVALID, slabs=empty)  # blocks, and no slabs
    assert "d_x" in err()
    group = pkg.Group([0])
    try:
        c.run(expect=INVALID, h=group._h)
        assert "aesw_theta_inputs_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.lookup_inputs(k, n_sets, None, None)
    finally:
        group.close()
    c.arena.check()
    assert c.untouched()
