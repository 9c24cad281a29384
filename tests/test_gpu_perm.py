"""libaesw_perm.so / Context.permuted_columns / Context.gather_fr on the GPU: plookup's permuted columns arranged from the lookup
multiplicities (tests/perm_cases.py).  Expected values come from tests/perm_model.py alone -- repeat and cumsum over the
histogram the kernels were given -- and plookup's four relations are checked on what the device wrote, without the model's
construction.  Histograms come from the accumulator on the device (K = 17 and K = 18 circuits, partly and fully filled, reference
and FIPS tables, PACKED adds plus the key add) and from perm_model.synthetic, uploaded.  d_a, d_s, the workspace and the report
always lie in poisoned, guard-banded buffers (tests/guarded.py): a call must touch nothing else, and rows n_rows ... 2^k - 1 of
every argument must keep the poison."""
import numpy as np
import pytest

import guarded as G
import perm_cases as pc
import perm_model as pm

pytestmark = pytest.mark.gpu

BINS = pm.BINS
OK, INVALID = 0, 1
PACKED = 1


@pytest.fixture(scope="module")
def worlds(pkg, ctx, oracle):
    other = pkg.Context(0, tables=oracle.fips_tables())
    yield {"reference": ctx, "fips": other}
    other.close()


_hists = {}


def circuit_histograms(pkg, ctx, which, k, n_sets, n, identical=False):
    """int32 [n_sets, BINS] on the device: n blocks of one circuit and its key slab through the accumulator, in two adds."""
    import torch
    at = (which, k, n_sets, n, identical)
    if at not in _hists:
        assert pkg.LAYOUT_PACKED == PACKED and n <= pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(k * 1000 + n)
        pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        if identical:
            pt[:] = pt[0]
        d_key, d_pt = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda(), torch.from_numpy(pt).cuda()
        kw = ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
        acc = ctx.multiplicity_accumulator(k, n_sets, PACKED).reset()
        half = n // 2
        for first, count in ((half, n - half), (0, half)):
            acc.add(first, ctx.encrypt_witness(d_pt[first:first + count], d_key, PACKED))
        acc.add_key(kw)
        assert acc.report() == {"lookups": 400 + 1056 * n, "misses": 0, "first_miss": None}
        _hists[at] = acc
    return _hists[at].histograms()


def composite(kinds, u, seed, zero_bin=0):
    """uint32[BINS]: the section of tag t from perm_model.synthetic(kinds[t]) (one kind for all: a string)"""
    rng = np.random.default_rng(seed)
    h = np.zeros(BINS, np.uint32)
    for tag in pm.TAGS:
        first, n = pm.SECTION[tag]
        kind = kinds if isinstance(kinds, str) else kinds.get(tag, "random")
        h[first:first + n] = pm.synthetic(kind, tag, u, rng)[first:first + n]
    h[pm.ZERO_ROW] = zero_bin
    return h


def upload(hists):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hists, np.uint32).view(np.int32)).cuda()


class Perm:
    """The C ABI on torch's current stream over guarded outputs, workspace and report."""

    def __init__(self, pkg, ctx, arena, k, n_sets, tag=""):
        import torch
        self.pkg, self.ctx, self.arena, self.k, self.n_sets, self.lib = pkg, ctx, arena, k, n_sets, pkg.api.load_perm_library()
        words = n_sets * 5 << k
        self.a, self.s = arena.out("a" + tag, words * 4), arena.out("s" + tag, words * 4)
        self.ws = arena.out("workspace" + tag, int(self.lib.aesw_perm_workspace_bytes(n_sets)))
        self.rep = arena.out("report" + tag, 24)
        self.torch = torch

    def build(self, mult, u, pad, expect=OK, h=None, k=None, n_sets=None, a=None, s=None, ws=None, rep=None, null=()):
        ptr = lambda name, t: None if name in null else t.data_ptr()  # noqa: E731
        rc = self.lib.aesw_perm_build_device(
            self.ctx._h if h is None else h, self.k if k is None else k, self.n_sets if n_sets is None else n_sets, u, pad, ptr("mult", mult),
            ptr("a", self.a if a is None else a), ptr("s", self.s if s is None else s), ptr("ws", self.ws if ws is None else ws),
            ptr("rep", self.rep if rep is None else rep), self.ctx._stream())
        assert rc == expect, (rc, self.ctx._lib.aesw_last_error(self.ctx._h))
        return rc

    def columns(self):
        """(a, s) uint32 [n_sets, 5, 2^k] on the host, guards checked"""
        self.torch.cuda.synchronize()
        self.arena.check()
        shape = (self.n_sets, 5, 1 << self.k)
        return [t.view(self.torch.int32).cpu().numpy().view(np.uint32).reshape(shape) for t in (self.a, self.s)]

    def report(self):
        return self.pkg.api.perm_report_dict(self.rep.view(self.torch.int64))

    def untouched(self):
        self.torch.cuda.synchronize()
        return all(self.arena.poisoned_on_device(t) for t in (self.a, self.s, self.ws, self.rep))


def verify(p, hists, u, pad, what="", only=None):
    """Every argument word for word against the model, the poison behind row u, the relations on the device's own output, the report."""
    a, s = p.columns()
    poison = np.uint32(int.from_bytes(bytes([p.arena.canary]) * 4, "little"))
    for st in range(p.n_sets):
        for tag in pm.TAGS:
            if only is not None and (st, tag) not in only:
                continue
            ea, es, _over = pm.arrange(hists[st], tag, u, pad)
            at = (what, st, tag, u, pad)
            for name, got, exp in (("A'", a[st, tag - 1], ea), ("S'", s[st, tag - 1], es)):
                bad = np.nonzero(got[:u] != exp)[0]
                assert not bad.size, "%s %r: %d positions differ, first %d: got %d, expected %d" % (name, at, bad.size, bad[0], got[bad[0]], exp[bad[0]])
                assert (got[u:] == poison).all(), "%s %r: a row at or behind n_rows was written" % (name, at)
            assert pm.relations(a[st, tag - 1, :u], s[st, tag - 1, :u], pm.counts(hists[st], tag, u)[0], u, pad) is None, at
    assert p.report() == pm.report(hists, u), (what, p.report())
    return a, s


REAL = ((17, 1, 95, "reference", (1 << 17) - 6, 0), (17, 2, 120, "fips", 1 << 17, pm.ZERO_ROW), (18, 3, 420, "reference", (1 << 18) - 6, 0))


@pytest.mark.parametrize("k,n_sets,n,which,u,pad", REAL)
def test_real_witnesses_word_for_word(pkg, worlds, k, n_sets, n, which, u, pad):
    ctx = worlds[which]
    mult = circuit_histograms(pkg, ctx, which, k, n_sets, n)
    hists = mult.cpu().numpy().view(np.uint32)
    assert int(hists.sum()) == 400 + 1056 * n and (n == pkg.block_capacity(k, n_sets)) == (n_sets == 1)
    for canary in G.CANARIES if k == 17 else G.CANARIES[:1]:
        p = Perm(pkg, ctx, G.DeviceArena(canary), k, n_sets)
        assert p.untouched()
        p.build(mult, u, pad)
        verify(p, hists, u, pad, "real")
    if n_sets == 1:  # the Python face: the default n_rows is 2^k
        a, s, rep = ctx.permuted_columns(k, n_sets, mult, pad_row=pad)
        a2, s2, rep2 = _hists[(which, k, n_sets, n, False)].permuted_columns(pad_row=pad)
        ea, es, _ = pm.arrange(hists[0], 2, 1 << k, pad)
        for got_a, got_s, r in ((a, s, rep), (a2, s2, rep2)):
            assert tuple(got_a.shape) == (1, 5, 1 << k) and r == {"arguments": 5, "overflowed": 0, "first_overflow": None}
            assert np.array_equal(got_a[0, 1].cpu().numpy(), ea) and np.array_equal(got_s[0, 1].cpu().numpy(), es)


@pytest.mark.parametrize("pad", pc.PAD_ROWS)
@pytest.mark.parametrize("u", pc.US)
def test_every_tail_of_n_rows(pkg, worlds, u, pad):
    ctx = worlds["fips"]
    real = circuit_histograms(pkg, ctx, "fips", 17, 2, 120).cpu().numpy().view(np.uint32)
    hists = np.stack([real[0], composite("random", u, seed=u)])
    p = Perm(pkg, ctx, G.DeviceArena(G.CANARIES[u % 2]), 17, 2)
    p.build(upload(hists), u, pad)
    verify(p, hists, u, pad, "tails")


def test_identical_blocks_one_run_over_many_workgroups(pkg, worlds):
    ctx = worlds["reference"]
    u = (1 << 17) - 6
    real = circuit_histograms(pkg, ctx, "reference", 17, 1, 95, identical=True).cpu().numpy().view(np.uint32)
    assert np.count_nonzero(real[512:66048]) <= 608 + 200
    one = composite({2: "one_bin"}, u, seed=3)  # one Xor bin holds all but 7 rows
    assert int(one[512:66048].max()) == u - 7
    hists = np.stack([real[0], one])
    p = Perm(pkg, ctx, G.DeviceArena(), 17, 2)
    p.build(upload(hists), u, 0)
    verify(p, hists, u, 0, "identical")


@pytest.mark.parametrize("kind", ("all_ones", "exact", "empty"))
def test_the_extremes_of_a_section(pkg, ctx, kind):
    """all_ones: D at its maximum, the leftover list at its shortest; exact: no all-zero run, the all-zero row is a leftover;
    empty: one run, and every table row a leftover."""
    u = (1 << 17) - 6
    hists = np.stack([composite(kind, u, seed=11), composite("random", u, seed=12)])
    p = Perm(pkg, ctx, G.DeviceArena(G.CANARIES[1]), 17, 2)
    p.build(upload(hists), u, 0)
    a, s = verify(p, hists, u, 0, kind)
    if kind == "exact":
        assert not (a[0, :, :u] == pm.ZERO_ROW).any() and ((s[0, :, :u] == pm.ZERO_ROW).sum(axis=1) == 1).all()
    if kind == "empty":
        assert (a[0, :, :u] == pm.ZERO_ROW).all()


def test_an_overflowing_section_is_clamped_and_reported(pkg, ctx):
    u = 1 << 17
    hists = np.stack([composite({4: "over_big"}, u, seed=21), composite({3: "over1"}, u, seed=22)])
    p = Perm(pkg, ctx, G.DeviceArena(), 17, 2)
    p.build(upload(hists), u, 0)
    verify(p, hists, u, 0, "overflow")
    assert p.report() == {"arguments": 10, "overflowed": 2, "first_overflow": (0, 4)}
    clean = np.stack([composite("random", u, seed=21), composite("random", u, seed=22)])  # the same shape without an overflow
    q = Perm(pkg, ctx, G.DeviceArena(), 17, 2, "_clean")
    q.build(upload(clean), u, 0)
    verify(q, clean, u, 0, "no overflow")
    assert q.report() == {"arguments": 10, "overflowed": 0, "first_overflow": None}


def test_the_report_over_more_arguments_than_its_workgroup_has_threads(pkg, ctx):
    """52 sets are 260 arguments: the 256 threads that write the report walk the overflow flags in two turns, and the one
    overflow there is arrives through an argument with an index of 256 or more."""
    u, n_sets = 1 << 17, 52
    plain = composite("random", u, seed=31)
    hists = np.stack([plain] * (n_sets - 1) + [composite({4: "over1"}, u, seed=32)])
    p = Perm(pkg, ctx, G.DeviceArena(), 17, n_sets)
    p.build(upload(hists), u, 0)
    verify(p, hists, u, 0, "260 arguments", only={(st, tag) for st in (0, n_sets - 1) for tag in pm.TAGS})
    assert (n_sets - 1) * 5 + 4 - 1 >= 256
    assert p.report() == {"arguments": 260, "overflowed": 1, "first_overflow": (n_sets - 1, 4)}


def test_a_pad_row_inside_the_section(pkg, ctx):
    u = 66564 + 1000
    hist = composite("random", u, seed=31)
    xor = hist[512:66048]
    used, unused = 512 + int(np.nonzero(xor)[0][100]), 512 + int(np.nonzero(xor == 0)[0][100])
    for pad in (used, unused):
        p = Perm(pkg, ctx, G.DeviceArena(), 17, 1, "_%d" % pad)
        p.build(upload(hist[None]), u, pad)
        a, s = verify(p, hist[None], u, pad, "pad row")
        assert int((s[0, 1, :u] == pad).sum()) == 1 + u - BINS


def test_garbage_outside_the_section_does_not_matter(pkg, ctx):
    u = (1 << 17) - 6
    rng = np.random.default_rng(41)
    dirty = np.stack([pm.synthetic("random", tag, u, rng) for tag in pm.TAGS])  # set t - 1: 0xffffffff outside the section of t
    clean = dirty.copy()
    for tag in pm.TAGS:
        first, n = pm.SECTION[tag]
        keep = clean[tag - 1, first:first + n].copy()
        clean[tag - 1] = 0
        clean[tag - 1, first:first + n] = keep
    assert (dirty[0, 256:] == 0xFFFFFFFF).all()
    p, q = Perm(pkg, ctx, G.DeviceArena(), 17, 5, "_dirty"), Perm(pkg, ctx, G.DeviceArena(G.CANARIES[1]), 17, 5, "_clean")
    p.build(upload(dirty), u, 0)
    q.build(upload(clean), u, 0)
    own = {(tag - 1, tag) for tag in pm.TAGS}
    a, s = verify(p, dirty, u, 0, "dirty")  # the other arguments of a dirty set overflow: the model clamps them alike
    b, t = verify(q, clean, u, 0, "clean", only=own)
    for st, tag in own:
        assert np.array_equal(a[st, tag - 1, :u], b[st, tag - 1, :u]) and np.array_equal(s[st, tag - 1, :u], t[st, tag - 1, :u])
    assert p.report()["overflowed"] == 20 and q.report()["overflowed"] == 0


def test_a_captured_build_rebuilds_on_every_replay(pkg, ctx):
    import torch
    u = (1 << 17) - 6
    hists = np.stack([composite("random", u, seed=51), composite({5: "over1"}, u, seed=52)])
    mult = upload(hists)
    arena = G.DeviceArena()
    p = Perm(pkg, ctx, arena, 17, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        p.build(mult, u, 0)
    torch.cuda.synchronize()
    assert p.untouched(), "the captured call ran during capture"
    for i in range(3):
        graph.replay()
        verify(p, hists, u, 0, "replay %d" % i)
        assert p.report()["overflowed"] == 1  # set by the call: a replay does not add to it
        arena.repoison()
        assert p.untouched()


def test_refusals_leave_the_outputs_alone_and_say_why(pkg, ctx):
    import torch
    p = Perm(pkg, ctx, G.DeviceArena(), 17, 1)
    mult = upload(composite("random", 1 << 17, seed=61)[None])
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    u = 1 << 17
    for k in (16, 2, 31):
        assert p.build(mult, u, 0, k=k, expect=INVALID) == INVALID and "aesw_perm_build_device" in err() and "k must be" in err()
    for n_sets in (0, 1025):
        assert p.build(mult, u, 0, n_sets=n_sets, expect=INVALID) == INVALID and "n_sets" in err()
    for rows in (66560, 0, u + 1, 0xFFFFFFFF):
        assert p.build(mult, rows, 0, expect=INVALID) == INVALID and "n_rows" in err()
    for pad in (66561, 0xFFFFFFFF):
        assert p.build(mult, u, pad, expect=INVALID) == INVALID and "pad_row" in err()
    for name, word in (("mult", "d_mult"), ("a", "d_a"), ("s", "d_s"), ("ws", "d_workspace"), ("rep", "d_report")):
        assert p.build(mult, u, 0, null=(name,), expect=INVALID) == INVALID and word in err(), name
    i32 = lambda t: t.view(torch.int32)  # noqa: E731
    assert p.build(i32(mult)[1:], u, 0, expect=INVALID) == INVALID and "d_mult" in err()  # 4-byte aligned only: never launched
    assert p.build(mult, u, 0, a=i32(p.a)[2:], expect=INVALID) == INVALID and "d_a" in err()
    assert p.build(mult, u, 0, s=i32(p.s)[1:], expect=INVALID) == INVALID and "d_s" in err()
    assert p.build(mult, u, 0, ws=p.ws[8:], expect=INVALID) == INVALID and "d_workspace" in err()
    assert p.build(mult, u, 0, rep=p.rep[4:], expect=INVALID) == INVALID and "d_report" in err()
    table, out = torch.zeros((BINS, 32), dtype=torch.uint8, device="cuda"), p.a[:64]
    gather = p.lib.aesw_perm_gather_fr_device
    assert gather(ctx._h, 2, None, table.data_ptr(), out.data_ptr(), ctx._stream()) == INVALID and "aesw_perm_gather_fr_device" in err() and "d_index" in err()
    assert gather(ctx._h, 2, mult.data_ptr(), table.view(-1)[8:].data_ptr(), out.data_ptr(), ctx._stream()) == INVALID and "d_table_fr" in err()
    assert gather(ctx._h, 2, mult.data_ptr(), table.data_ptr(), p.a[8:].data_ptr(), ctx._stream()) == INVALID and "d_out_fr" in err()
    assert gather(ctx._h, (1 << 36) + 1, mult.data_ptr(), table.data_ptr(), out.data_ptr(), ctx._stream()) == INVALID and "n_cells" in err()
    assert gather(ctx._h, 0, None, None, None, ctx._stream()) == OK  # nothing to gather: nothing is launched, whatever is missing
    group = pkg.Group([0])
    try:
        assert p.build(mult, u, 0, h=group._h, expect=INVALID) == INVALID and "aesw_perm_build_device" in err(group)
        assert gather(group._h, 2, mult.data_ptr(), table.data_ptr(), out.data_ptr(), ctx._stream()) == INVALID and "aesw_perm_gather_fr_device" in err(group)
        with pytest.raises(pkg.AeswError) as e:
            group.permuted_columns(17, 1, mult)
        assert e.value.status == pkg.api.ERR_INVALID_ARG
    finally:
        group.close()
    p.arena.check()
    assert p.untouched()
    with pytest.raises(pkg.AeswError) as e:  # the Python face ends in the same refusals
        ctx.permuted_columns(17, 1, mult, n_rows=66560)
    assert e.value.status == pkg.api.ERR_INVALID_ARG and "n_rows" in str(e.value)
    with pytest.raises(ValueError):
        ctx.permuted_columns(17, 2, mult)


@pytest.mark.parametrize("mode", pc.STORE_MODES)
def test_gather_fr_is_a_table_lookup(pkg, worlds, mode):
    import torch
    ctx = worlds["reference"]
    rng = np.random.default_rng(70 + mode)
    table = rng.integers(0, 256, (BINS, 32), dtype=np.uint8)
    d_table = torch.from_numpy(table).cuda()
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        lib = pkg.api.load_perm_library()
        for n in pc.GATHER_CELLS:
            arena = G.DeviceArena(G.CANARIES[n % 2])
            index = rng.integers(0, BINS, n, dtype=np.uint32)
            planted = {0: 66561, n // 2: 0xFFFFFFFF, n - 1: 66560} if n > 2 else {0: 0xFFFFFFFF if mode else 66561}
            for at, v in planted.items():
                index[at] = v
            d_index = arena.input("index", index.view(np.uint8)).view(torch.int32)  # 4-byte aligned only
            out = arena.out("fr", n * 32, (n, 32))
            rc = lib.aesw_perm_gather_fr_device(ctx._h, n, d_index.data_ptr(), d_table.data_ptr(), out.data_ptr(), ctx._stream())
            assert rc == OK, ctx._lib.aesw_last_error(ctx._h)
            torch.cuda.synchronize()
            arena.check()
            exp = np.where((index < BINS)[:, None], table[np.minimum(index, BINS - 1)], 0).astype(np.uint8)
            G.assert_bytes("gather n = %d" % n, out.cpu().numpy(), exp)
            assert not exp[[at for at, v in planted.items() if v >= BINS]].any()
    finally:
        ctx.set_option("fr_store_mode", before)


def test_the_gathered_columns_keep_the_relations_as_fr_bytes(pkg, worlds):
    """A' and S' of a real witness through the Python face, gathered through an injective table of random cells: the relations
    on the 32-byte cells are the relations on the rows."""
    import torch
    ctx = worlds["reference"]
    k, u, pad = 17, (1 << 17) - 6, 0
    mult = circuit_histograms(pkg, ctx, "reference", k, 1, 95)
    a, s, rep = ctx.permuted_columns(k, 1, mult, n_rows=u, pad_row=pad)
    assert rep["overflowed"] == 0
    rng = np.random.default_rng(80)
    table = rng.integers(0, 256, (BINS, 32), dtype=np.uint8)
    table[:, :4] = np.arange(BINS, dtype=np.uint32).view(np.uint8).reshape(BINS, 4)  # no two rows alike
    d_table = torch.from_numpy(table).cuda()
    fa = ctx.gather_fr(a[0, :, :u].contiguous(), d_table).cpu().numpy()
    fs = ctx.gather_fr(s[0, :, :u].contiguous(), d_table).cpu().numpy()
    assert fa.shape == (5, u, 32)
    hist = mult.cpu().numpy().view(np.uint32)[0]
    column = table[pm.table_column(u, pad)]

    def key(cells):  # the cells as a sorted multiset
        w = np.ascontiguousarray(cells).view(np.uint64).reshape(-1, 4)
        return w[np.lexsort(w.T[::-1])]
    for tag in pm.TAGS:
        A, S = fa[tag - 1], fs[tag - 1]
        c, _ = pm.counts(hist, tag, u)
        assert np.array_equal(key(A), key(table[np.repeat(np.arange(BINS), c)])), tag  # a permutation of the inputs
        assert np.array_equal(key(S), key(column)), tag                              # a permutation of the table column
        same_as_table, same_as_prev = (A == S).all(axis=1), np.concatenate([[False], (A[1:] == A[:-1]).all(axis=1)])
        assert same_as_table[0] and (same_as_table | same_as_prev).all(), tag
