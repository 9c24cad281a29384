"""libaesw_acc.so / Context.multiplicity_accumulator on the GPU: the lookup multiplicities of one circuit accumulated over
several calls (tests/acc_cases.py).  The yardstick is tests/mult_model.py over the ORACLE's circuit -- the advice and selector
columns of its restated synthesize() for the same key and plaintexts -- which shares nothing with the kernels; below K = 11
the oracle holds no circuit (it needs the key schedule's 1 760 rows), and the model reads the product's assembled columns and
selectors instead, as tests/test_gpu_mult.py does.  d_mult and the report always lie in poisoned, guard-banded buffers
(tests/guarded.py): a call must touch nothing else."""
import ctypes as C

import numpy as np
import pytest

import acc_cases as ac
import guarded as G
import mult_model as mm

pytestmark = pytest.mark.gpu

BINS = mm.BINS
OK, INVALID, CAPACITY = 0, 1, 5


@pytest.fixture(scope="module")
def worlds(pkg, ctx, oracle):
    """tables name -> (context, oracle with the same tables)"""
    import oracle_lib
    fips = oracle.fips_tables()
    other = pkg.Context(0, tables=fips)
    yield {"reference": (ctx, oracle), "fips": (other, oracle_lib.Oracle(tables=fips))}
    other.close()


_expected = {}


def expected(pkg, ctx, orc, k, n_sets, key, pt):
    """(hist int64[n_sets, BINS] of the whole circuit with its key rows, the same without them): computed once per circuit."""
    at = (id(orc), k, n_sets, key.tobytes(), pt.tobytes())
    if at not in _expected:
        tables = orc.tables()
        if k >= 11:
            with orc.circuit(k, n_sets, key, pt, record_copies=False) as c:
                assert c.status == 0
                adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
                sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
        else:
            import torch
            assert len(pt) == 0
            kw = ctx.key_schedule_witness(torch.from_numpy(key.reshape(1, 16)).cuda(), ac.PACKED, want_rk=False)
            adv = ctx.assemble_advice_circuits(k, n_sets, ctx.alloc_witness(1, ac.PACKED), kw, [0], as_fr=False, layout=ac.PACKED, n_blocks=0).cpu().numpy()[0]
            sel, _fixed = pkg.assemble_selectors(k, n_sets, 0)
        whole, misses = mm.multiplicities(adv, sel, tables)
        assert misses == 0
        no_key = sel.copy()
        no_key[:5, :pkg.KEY_ROWS] = 0  # the key rows lie in front of set 0's blocks: its five selectors
        blocks, _ = mm.multiplicities(adv, no_key, tables)
        assert int(blocks.sum()) == 1056 * len(pt) and int(whole.sum() - blocks.sum()) == (400 if k >= 9 else 0)
        whole.setflags(write=False)
        blocks.setflags(write=False)
        _expected[at] = (whole, blocks)
    return _expected[at]


class Circuit:
    """One circuit on the device: n blocks under one key and the key's slab."""

    def __init__(self, pkg, ctx, layout, k, n_sets, n, seed=0, identical=False):
        import torch
        self.pkg, self.ctx, self.layout, self.k, self.n_sets, self.n = pkg, ctx, layout, k, n_sets, n
        rng = np.random.default_rng(seed)
        self.key = rng.integers(0, 256, 16, dtype=np.uint8)
        self.pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        if identical:
            self.pt[:] = self.pt[0]
        self.d_key, self.d_pt = torch.from_numpy(self.key).cuda(), torch.from_numpy(self.pt).cuda()
        self.kw = ctx.key_schedule_witness(self.d_key.reshape(1, 16), layout, want_rk=False)
        self.wit = ctx.encrypt_witness(self.d_pt, self.d_key, layout) if n else ctx.alloc_witness(1, layout)
        self.st = [pkg.column_stride(layout, i) for i in range(3)]
        torch.cuda.synchronize()

    def slabs(self, first, count):
        """(x, y, z) views of blocks [first, first + count)"""
        return [t[first * s:(first + count) * s] for t, s in zip(self.wit[:3], self.st)]


class Acc:
    """The C ABI on torch's current stream over one guarded histogram buffer and one guarded report."""

    def __init__(self, circ, arena, tag=""):
        import torch
        self.c, self.arena, self.lib = circ, arena, circ.pkg.api.load_acc_library()
        self.mult = arena.out("mult" + tag, circ.n_sets * BINS * 4)
        self.rep = arena.out("report" + tag, 24)
        assert untouched(arena, self.mult, self.rep)
        self.mult32 = self.mult.view(torch.int32).view(circ.n_sets, BINS)

    def _done(self, rc, expect):
        ctx = self.c.ctx
        assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
        return rc

    def reset(self, expect=OK, mult=None, h=None, n_sets=None):
        c = self.c
        return self._done(self.lib.aesw_acc_reset_device(c.ctx._h if h is None else h, c.n_sets if n_sets is None else n_sets,
                                                         (self.mult if mult is None else mult).data_ptr(), self.rep.data_ptr(), c.ctx._stream()), expect)

    def add(self, first, count, chunk=0, slabs=None, expect=OK, layout=None, k=None, mult=None, h=None):
        c = self.c
        x, y, z = c.slabs(first, count) if slabs is None else slabs
        return self._done(self.lib.aesw_acc_add_device_chunk(
            c.ctx._h if h is None else h, c.k if k is None else k, c.n_sets, first, count, c.layout if layout is None else layout, x.data_ptr(), y.data_ptr(),
            z.data_ptr(), (self.mult if mult is None else mult).data_ptr(), self.rep.data_ptr(), c.ctx._stream(), chunk), expect)

    def add_key(self, expect=OK, layout=None, k=None, h=None):
        c = self.c
        ks = c.pkg.api.KeySlab(None, *[t.data_ptr() for t in c.kw[1:4]])
        return self._done(self.lib.aesw_acc_add_key_device(c.ctx._h if h is None else h, c.k if k is None else k, c.layout if layout is None else layout,
                                                           C.byref(ks), self.mult.data_ptr(), self.rep.data_ptr(), c.ctx._stream()), expect)

    def result(self):
        """(hist int64 [n_sets, BINS], report dict), guards checked"""
        import torch
        torch.cuda.synchronize()
        self.arena.check()
        return self.mult32.cpu().numpy().astype(np.int64), self.c.pkg.api.mult_report_dict(self.rep.view(torch.int64))


def untouched(arena, *tensors):
    """Every byte of every tensor still holds the arena's canary."""
    import torch
    return all(arena.poisoned(t.contiguous().view(torch.uint8)) for t in tensors)


def same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert not bad.size, "%s: %d bins differ, first (set, bin) = %s: got %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def clean(k, n):
    return {"lookups": (400 if k >= 9 else 0) + 1056 * n, "misses": 0, "first_miss": None}


@pytest.mark.parametrize("tables", ac.TABLE_SETS)
@pytest.mark.parametrize("layout", ac.LAYOUTS)
@pytest.mark.parametrize("k,n_sets,n", ac.SHAPES)
def test_every_cut_of_a_circuit_equals_the_model(pkg, worlds, k, n_sets, n, layout, tables):
    import torch
    ctx, orc = worlds[tables]
    assert n <= pkg.block_capacity(k, n_sets)
    c = Circuit(pkg, ctx, layout, k, n_sets, n, seed=k * 10 + n_sets)
    exp, exp_blocks = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    runs = ac.ragged(n)
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

    # the same adds out of ONE slab buffer: generate, add, overwrite
    a = Acc(c, arenas[0], "_reuse")
    a.reset()
    longest = max([count for _f, count in runs] + [1])
    buf = ctx.alloc_witness(longest, layout)
    for first, count in runs:
        ctx.encrypt_witness(c.d_pt[first:first + count], c.d_key, layout, out=buf)
        a.add(first, count, slabs=buf[:3])
    got, rep = a.result()
    same(got, exp_blocks, "one slab buffer")
    assert rep == {"lookups": 1056 * n, "misses": 0, "first_miss": None}, rep

    # several pairs of workgroups add into the same bins; from LONG_FROM blocks on also chunks longer than one round of the waves
    for chunk in ac.FORCED_CHUNKS + (ac.LONG_CHUNKS if n >= ac.LONG_FROM else ()):
        a = Acc(c, arenas[1], "_chunk%d" % chunk)
        a.reset(), a.add_key(), a.add(0, n, chunk=chunk)
        got, rep = a.result()
        same(got, exp, "chunk %d" % chunk)
        assert rep == clean(k, n), rep

    if (k, n_sets, layout) == (14, 3, ac.PACKED):  # the Python face, and the one-shot call over the same circuit
        acc = ctx.multiplicity_accumulator(k, n_sets, layout)
        acc.reset()
        for first, count in runs:
            acc.add(first, pkg.Witness(*c.slabs(first, count), None, None))
        acc.add_key(c.kw)
        assert acc.report() == clean(k, n)
        hist = acc.histograms()
        assert tuple(hist.shape) == (n_sets, BINS) and str(hist.dtype) == "torch.int32"
        same(hist.cpu().numpy().astype(np.int64), exp, "Context.multiplicity_accumulator")
        mult, rep = ctx.lookup_multiplicities(k, n_sets, c.wit, c.kw, [n], layout=layout)
        same(mult.cpu().numpy().astype(np.int64)[0], exp, "Context.lookup_multiplicities")
        assert rep == clean(k, n)
    torch.cuda.synchronize()


def test_identical_blocks_count_exactly(pkg, worlds):
    """Every block the same: all workgroups add to the same few hundred words."""
    ctx, orc = worlds["reference"]
    k, n_sets, n, chunk = ac.CONTENTION
    c = Circuit(pkg, ctx, ac.PACKED, k, n_sets, n, seed=5, identical=True)
    exp, _ = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    assert np.count_nonzero(exp[1]) <= 1056 and exp[1].max() >= 12
    a = Acc(c, G.DeviceArena())
    a.reset(), a.add(0, n, chunk=chunk), a.add_key()
    got, rep = a.result()
    same(got, exp, "identical blocks")
    assert rep == clean(k, n)


def many_sets_expectation(pkg, orc, key, pt):
    """{set: int64[BINS]} after ac.MANY_RUNS, the runs' blocks being those of `pt` in the order of the runs.  The histogram of a
    block does not depend on where a circuit places it: mult_model's block_histograms over the oracle's K = 14 / N = 3 circuit of
    the same key and plaintexts; the set of a circuit block is the product's placement (held against the oracle's in
    tests/test_placement.py)."""
    k, n_sets = ac.MANY_SETS
    assert len(pt) == sum(count for _first, count in ac.MANY_RUNS) <= pkg.block_capacity(14, 3)
    with orc.circuit(14, 3, key, pt, record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * 3 + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * 3 + 1)])
        places = [c.block_placement(b) for b in range(len(pt))]
    h, misses = mm.block_histograms(adv, sel, orc.tables(), places)
    assert not misses.any() and h.sum(axis=1).tolist() == [1056] * len(pt)
    exp, at = {}, 0
    for first, count in ac.MANY_RUNS:
        for j in range(count):
            s = pkg.block_placement(k, n_sets, first + j)[0]
            exp[s] = exp.get(s, 0) + h[at]
            at += 1
    assert tuple(sorted(exp)) == ac.MANY_TOUCHED
    return exp


def check_many_sets(a, exp, n):
    """The histograms of a.mult32 [n_sets, BINS] are `exp` in its sets and zero in every other one -- looked at on the device, only
    the sets of `exp` are copied to the host --, the report is clean over n blocks, the guards are intact."""
    import torch
    a.arena.check_on_device()
    touched = sorted(exp)
    busy = torch.nonzero((a.mult32 != 0).any(dim=1)).flatten().tolist()
    assert busy == touched, "sets with a count: %s, expected %s" % (busy[:16], touched)
    got = a.mult32[torch.as_tensor(touched, device=a.mult32.device)].cpu().numpy().astype(np.int64)
    same(got, np.stack([exp[s] for s in touched]), "the sets %s" % (touched,))
    rep = a.c.pkg.api.mult_report_dict(a.rep.view(torch.int64))
    assert rep == {"lookups": 1056 * n, "misses": 0, "first_miss": None}, rep


@pytest.mark.parametrize("layout", ac.LAYOUTS)
def test_a_circuit_of_1024_sets(pkg, worlds, layout):
    """n_sets at its bound: runs that start and end deep inside the set index, each add out of slab views of its own."""
    ctx, orc = worlds["reference"]
    k, n_sets = ac.MANY_SETS
    assert pkg.block_capacity(k, n_sets) == 3070
    c = Circuit(pkg, ctx, layout, k, n_sets, 16, seed=1024)
    exp = many_sets_expectation(pkg, orc, c.key, c.pt)
    a = Acc(c, G.DeviceArena(), "_many")
    a.reset()
    at = 0
    for first, count in ac.MANY_RUNS:
        a.add(first, count, slabs=c.slabs(at, count))  # slab i of a run is block first + i
        at += count
    check_many_sets(a, exp, 16)


def test_one_run_through_all_1024_sets(pkg, worlds):
    """One add of all 3 070 blocks: a grid 1 024 pieces high.  The yardstick is mult_model's block_histograms over the columns the
    product assembles for the same blocks at K = 22 / N = 1 (3 082 blocks in one set), every bin of every set compared."""
    import torch
    ctx, _orc = worlds["reference"]
    k, n_sets = ac.MANY_SETS
    n = pkg.block_capacity(k, n_sets)
    assert n == 3070 <= pkg.block_capacity(22, 1)
    c = Circuit(pkg, ctx, ac.PACKED, k, n_sets, n, seed=3070)
    adv = ctx.assemble_advice_circuits(22, 1, c.wit, c.kw, [n], as_fr=False, layout=ac.PACKED, n_blocks=n).cpu().numpy()[0]
    sel, _fixed = pkg.assemble_selectors(22, 1, n)
    sets = [pkg.block_placement(k, n_sets, b)[0] for b in range(n)]
    assert sets == [0] + [1 + (b - 1) // 3 for b in range(1, n)]
    places = {}  # set of the K = 12 circuit -> where the K = 22 circuit placed its blocks: set s >= 1 holds blocks 1 + 3 (s - 1) ... 3 + 3 (s - 1)
    for b in range(n):
        places.setdefault(sets[b], []).append(pkg.block_placement(22, 1, b))
    exp = np.zeros((n_sets, BINS), np.int32)
    for s in range(n_sets):
        h, misses = mm.block_histograms(adv, sel, ctx._tables, places[s])
        assert not misses.any()
        exp[s] = h.sum(axis=0)
    assert int(exp.sum(dtype=np.int64)) == 1056 * n
    a = Acc(c, G.DeviceArena(G.CANARIES[1]), "_all")
    a.reset(), a.add(0, n)
    a.arena.check_on_device()
    want = torch.from_numpy(exp).cuda()
    bad = torch.nonzero(a.mult32 != want)
    assert not bad.numel(), "%d bins differ, first (set, bin) = %s: got %d, expected %d" % (
        len(bad), bad[0].tolist(), int(a.mult32[tuple(bad[0])]), int(want[tuple(bad[0])]))
    rep = pkg.api.mult_report_dict(a.rep.view(torch.int64))
    assert rep == {"lookups": 1056 * n, "misses": 0, "first_miss": None}, rep


def test_misses_are_counted_named_and_left_out_of_the_bins(pkg, worlds):
    import torch
    ctx, orc = worlds["reference"]
    k, n_sets, n, layout = 14, 3, 34, ac.PACKED
    c = Circuit(pkg, ctx, layout, k, n_sets, n, seed=77)
    exp, _ = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
    py = pkg.packed_index(1)
    tags = pkg.selector_tags()[0]
    runs = ac.ragged(n)  # (0, 1), (1, 7), (8, 16), (24, 10)

    def sbox_cell(blk, row):
        """(index into y of the row's output, the bin the lookup would have hit)"""
        assert tags[row] == 3
        return blk * c.st[1] + int(py[row]), 256 + int(c.wit.x[blk * c.st[0] + row])

    # one flipped y byte of an S-box row in the second add: block 1 + 4 of the circuit, set 0
    at, lost = sbox_cell(5, 37)
    c.wit.y[at] ^= 0x40
    torch.cuda.synchronize()
    a = Acc(c, G.DeviceArena(), "_one")
    a.reset(), a.add_key()
    for first, count in runs:
        a.add(first, count)
    got, rep = a.result()
    assert rep == {"lookups": 400 + 1056 * n, "misses": 1, "first_miss": (5, False, 37)}, rep
    diff = exp - got
    assert diff.sum() == 1 and diff[0, lost] == 1 and np.count_nonzero(diff) == 1
    # a second miss in a later add (block 30, set 2): the first one is the smaller, whichever add came first
    row2 = int(np.nonzero(np.asarray(tags) == 3)[0][-1])  # the last S-box row of a block
    at2, lost2 = sbox_cell(30, row2)
    c.wit.y[at2] ^= 0x01
    torch.cuda.synchronize()
    want = exp.copy()
    want[0, lost] -= 1
    want[2, lost2] -= 1
    for order in (runs, runs[::-1]):
        a = Acc(c, G.DeviceArena(G.CANARIES[1]), "_two")
        a.reset()
        for first, count in order:
            a.add(first, count, chunk=3)
        a.add_key()
        got, rep = a.result()
        same(got, want, "two misses")
        assert rep == {"lookups": 400 + 1056 * n, "misses": 2, "first_miss": (5, False, 37)}, rep
    # the later one alone: it is named with the circuit's block index, not the slab's
    c.wit.y[at] ^= 0x40
    torch.cuda.synchronize()
    a = Acc(c, G.DeviceArena(), "_late")
    a.reset(), a.add(24, 10)
    _got, rep = a.result()
    assert rep == {"lookups": 1056 * 10, "misses": 1, "first_miss": (30, False, row2)}, rep


@pytest.mark.parametrize("k,gain", ((14, 400), (9, 400), (8, 0)))
def test_the_key_slab_adds_its_400_rows_to_set_0(pkg, worlds, k, gain):
    ctx, _orc = worlds["reference"]
    n_sets = 2 if k == 14 else 1
    for layout in ac.LAYOUTS:
        c = Circuit(pkg, ctx, layout, k, n_sets, 0, seed=k)
        a = Acc(c, G.DeviceArena())
        a.reset(), a.add_key()
        got, rep = a.result()
        sums = mm.section_sums(got)
        assert sums[0].tolist() == ([160, 200, 40, 0, 0] if gain else [0] * 5) and not sums[1:].any() and not got[:, BINS - 1].any()
        assert rep == {"lookups": gain, "misses": 0, "first_miss": None}
    # a miss in the key slab names unit 0 with the key-slab bit
    if k == 14:
        import torch
        ktags = pkg.selector_tags()[1]
        assert ktags[42] == 3
        c.kw.ky[int(pkg.key_packed_index(1)[42])] ^= 0x40
        torch.cuda.synchronize()
        a = Acc(c, G.DeviceArena())
        a.reset(), a.add_key()
        got, rep = a.result()
        assert rep == {"lookups": 400, "misses": 1, "first_miss": (0, True, 42)} and int(got.sum()) == 399


def test_captured_calls_replay_and_captured_adds_accumulate(pkg, worlds):
    import torch
    ctx, orc = worlds["reference"]
    k, n_sets, n = 14, 3, 34
    c = Circuit(pkg, ctx, ac.PACKED, k, n_sets, n, seed=14)
    exp, exp_blocks = expected(pkg, ctx, orc, k, n_sets, c.key, c.pt)
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
    c = Circuit(pkg, ctx, ac.PACKED, 12, 2, 3, seed=3)
    arena = G.DeviceArena()
    a = Acc(c, arena)
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    assert a.add(0, 3, layout=ac.VALUES, expect=INVALID) == INVALID and "aesw_acc_add_device" in err() and "VALUES" in err()
    assert a.add_key(layout=ac.VALUES, expect=INVALID) == INVALID and "aesw_acc_add_key_device" in err() and "VALUES" in err()
    for k in (1, 31):
        assert a.add(0, 1, k=k, expect=INVALID) == INVALID and "k must be" in err()
        assert a.add_key(k=k, expect=INVALID) == INVALID and "k must be" in err()
    flat = a.mult.view(torch.int32)
    assert a.add(0, 3, mult=flat[1:], expect=INVALID) == INVALID and "d_mult" in err()  # 4-byte aligned only
    assert a.reset(mult=flat[1:], expect=INVALID) == INVALID and "aesw_acc_reset_device" in err() and "d_mult" in err()
    assert a.reset(n_sets=0, expect=INVALID) == INVALID and "n_sets" in err()
    group = pkg.Group([0])
    try:
        for rc in (a.reset(h=group._h, expect=INVALID), a.add(0, 3, h=group._h, expect=INVALID), a.add_key(h=group._h, expect=INVALID)):
            assert rc == INVALID and "aesw_acc_" in err(group)
        with pytest.raises(pkg.AeswError) as e:
            group.multiplicity_accumulator(12, 2)
        assert e.value.status == pkg.api.ERR_INVALID_ARG
    finally:
        group.close()
    torch.cuda.synchronize()
    assert untouched(arena, a.mult, a.rep)
    # over the capacity (K = 12, N = 2 holds 1 + 3 blocks): nothing is enqueued, d_mult stays bit-identical
    a.reset(), a.add(0, 3)
    before, rep_before = a.result()
    bytes_before = a.mult.cpu().numpy().copy()
    big = ctx.alloc_witness(8, ac.PACKED)
    for first, count in ((2, 3), (0, 5), (4, 1), (5, 0), (1 << 63, 1 << 63)):
        assert a.add(first, count, slabs=big[:3], expect=CAPACITY) == CAPACITY and "aesw_acc_add_device" in err() and "capacity" in err()
    assert a.add(4, 0, slabs=big[:3]) == OK  # an empty run at the very end is one
    got, rep = a.result()
    assert np.array_equal(a.mult.cpu().numpy(), bytes_before) and rep == rep_before and np.array_equal(got, before)
    with pytest.raises(pkg.AeswError) as e:
        ctx.multiplicity_accumulator(12, 2, ac.VALUES).reset().add(0, pkg.Witness(*big[:3], None, None), n_blocks=1)
    assert e.value.status == pkg.api.ERR_INVALID_ARG
    with pytest.raises(pkg.AeswError) as e:
        ctx.multiplicity_accumulator(12, 2).reset().add(3, pkg.Witness(*big[:3], None, None), n_blocks=2)
    assert e.value.status == pkg.api.ERR_CAPACITY
