"""aesw_mult_count_device / Context.lookup_multiplicities on the GPU: the lookup multiplicities of a many-circuit batch, both
forms (tests/mult_cases.py).  The yardstick is tests/mult_model.py applied to what the prover holds -- the advice columns
assemble_advice_circuits writes, as bytes, and the selector columns of assemble_selectors -- which shares neither slab indexing
nor placement arithmetic with the kernels.  d_mult and the report always lie in poisoned, guard-banded buffers
(tests/guarded.py): the call must set all it owns and touch nothing else."""
import ctypes as C

import numpy as np
import pytest

import circuit_cases as cc
import guarded as G
import mult_cases as mc
import mult_model as mm

pytestmark = pytest.mark.gpu

BINS = mm.BINS


@pytest.fixture(scope="module")
def contexts(pkg, ctx):
    other = pkg.Context(0, tables=G.random_tables())
    yield {"reference": ctx, "random": other}
    other.close()


class Batch:
    """C circuits on the device: the blocks' witness under each block's circuit key (keys / pt given or random), C key slabs."""

    def __init__(self, pkg, ctx, layout, k, n_sets, counts, seed=0, keys=None, pt=None):
        import torch
        self.pkg, self.ctx, self.layout, self.k, self.n_sets = pkg, ctx, layout, k, n_sets
        self.counts = [int(c) for c in counts]
        self.nc, self.n = len(counts), int(sum(counts))
        self.offs = pkg.circuit_offsets(k, n_sets, counts, self.n)
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 256, (self.nc, 16), dtype=np.uint8) if keys is None else keys
        pt = rng.integers(0, 256, (self.n, 16), dtype=np.uint8) if pt is None else pt
        self.keys, self.pt = torch.from_numpy(keys).cuda(), torch.from_numpy(pt).cuda()
        self.kw = ctx.key_schedule_witness(self.keys, layout, want_rk=False)
        per_block = torch.repeat_interleave(self.keys, torch.as_tensor(self.counts, dtype=torch.int64, device="cuda"), dim=0)
        self.wit = ctx.encrypt_witness(self.pt, per_block, layout, want_ct=False) if self.n else ctx.alloc_witness(1, layout, want_ct=False)
        self.d_offs = torch.from_numpy(self.offs.view(np.int64)).cuda()
        torch.cuda.synchronize()

    def raw(self, mult, report, form, key_slabs=True, layout=None, k=None, expect=0, offsets=None):
        """The test-facing C entry point on torch's current stream; returns the status.  offsets: a device tensor of C + 1 int64 in
        place of the batch's own."""
        lib, ctx = self.pkg.api.load_mult_library(), self.ctx
        ks = self.pkg.api.KeySlab(*[t.data_ptr() for t in self.kw[:4]])
        d_offs = self.d_offs if offsets is None else offsets
        assert str(d_offs.dtype) == "torch.int64" and d_offs.is_cuda and d_offs.numel() == self.nc + 1
        rc = lib.aesw_mult_count_device_form(
            ctx._h, self.k if k is None else k, self.n_sets, self.nc, d_offs.data_ptr(), self.layout if layout is None else layout,
            self.wit.x.data_ptr(), self.wit.y.data_ptr(), self.wit.z.data_ptr(), C.byref(ks) if key_slabs else None,
            mult.data_ptr(), report.data_ptr(), ctx._stream(), form)
        assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
        return rc

    def outputs(self, arena, tag=""):
        import torch
        mult = arena.out("mult" + tag, self.nc * self.n_sets * BINS * 4)
        rep = arena.out("report" + tag, 24)
        assert untouched(arena, mult, rep)
        return mult.view(torch.int32).view(self.nc, self.n_sets, BINS), rep

    def count(self, arena, form, **kw):
        """(mult as int64 numpy [C, N, BINS], report dict) of one call into fresh poisoned buffers, guards checked."""
        import torch
        mult, rep = self.outputs(arena, "_%d" % form)
        self.raw(mult, rep, form, **kw)
        torch.cuda.synchronize()
        arena.check()
        return mult.cpu().numpy().astype(np.int64), self.pkg.api.mult_report_dict(rep.view(torch.int64))

    def expected(self, key_slabs=True):
        """(hist [C, N, BINS], misses) by the numpy model over the assembled byte columns and the selectors."""
        pkg, ctx = self.pkg, self.ctx
        adv = ctx.assemble_advice_circuits(self.k, self.n_sets, self.wit, self.kw, self.counts, as_fr=False, layout=self.layout,
                                           n_blocks=self.n).cpu().numpy()
        hist, misses = np.zeros((self.nc, self.n_sets, BINS), np.int64), 0
        for c in range(self.nc):
            sel, _fixed = pkg.assemble_selectors(self.k, self.n_sets, self.counts[c])
            if not key_slabs:
                sel[:5, :pkg.KEY_ROWS] = 0  # the key rows lie in front of set 0's blocks: its five selectors
            hist[c], m = mm.multiplicities(adv[c], sel, ctx._tables)
            misses += m
        return hist, misses

    def parts(self):
        """(h int64[n, BINS], kh int64[C, BINS]): what every slab block and every key slab looks up, by mult_model's block_histograms
        and key_histogram over the assembled byte columns and the selectors of the batch as its own offsets cut it."""
        pkg, ctx = self.pkg, self.ctx
        adv = ctx.assemble_advice_circuits(self.k, self.n_sets, self.wit, self.kw, self.counts, as_fr=False, layout=self.layout,
                                           n_blocks=self.n).cpu().numpy()
        h, kh = np.zeros((self.n, BINS), np.int64), np.zeros((self.nc, BINS), np.int64)
        for c in range(self.nc):
            sel, _fixed = pkg.assemble_selectors(self.k, self.n_sets, self.counts[c])
            places = [pkg.block_placement(self.k, self.n_sets, j) for j in range(self.counts[c])]
            at = int(self.offs[c])
            h[at:at + self.counts[c]], misses = mm.block_histograms(adv[c], sel, ctx._tables, places)
            kh[c], key_misses = mm.key_histogram(adv[c], sel, ctx._tables)
            assert not misses.any() and key_misses == 0
        assert h.sum(axis=1).tolist() == [1056] * self.n and kh.sum(axis=1).tolist() == [400] * self.nc
        return h, kh


def untouched(arena, *tensors):
    """Every byte of every tensor still holds the arena's canary."""
    import torch
    return all(arena.poisoned(t.contiguous().view(torch.uint8)) for t in tensors)


def same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert not bad.size, "%s: %d bins differ, first (c, s, bin) = %s: got %d, expected %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("tables", mc.TABLE_SETS)
@pytest.mark.parametrize("layout", mc.LAYOUTS)
@pytest.mark.parametrize("k,n_sets,nc", mc.SHAPES)
def test_parity_over_the_circuit_shapes(pkg, contexts, k, n_sets, nc, layout, tables):
    ctx = contexts[tables]
    cap, cap0 = pkg.block_capacity(k, n_sets), pkg.block_capacity(k, 1)
    counts = cc.ragged_counts(cap, cap0, n_sets, nc, np.random.default_rng(k * 100 + n_sets * 10 + nc))
    b = Batch(pkg, ctx, layout, k, n_sets, counts, seed=k + layout)
    exp, misses = b.expected()
    total = (400 * nc if (1 << k) >= 400 else 0) + 1056 * b.n  # below K = 9 a circuit has no room for the key rows: no selector is on
    assert misses == 0 and int(exp.sum()) == total
    for canary, form in zip(G.CANARIES, mc.FORMS):
        got, rep = b.count(G.DeviceArena(canary), form)
        same(got, exp, "form %d" % form)
        assert rep == {"lookups": total, "misses": 0, "first_miss": None}, rep
    if (k, n_sets, nc) == (13, 3, 3):  # without key slabs, and through the Python face (the default form)
        exp_nk, _ = b.expected(key_slabs=False)
        for form in mc.FORMS:
            got, rep = b.count(G.DeviceArena(), form, key_slabs=False)
            same(got, exp_nk, "no key slabs, form %d" % form)
            assert rep["lookups"] == 1056 * b.n and rep["misses"] == 0
        mult, rep = ctx.lookup_multiplicities(k, n_sets, b.wit, b.kw, counts, layout=layout)
        same(mult.cpu().numpy().astype(np.int64), exp, "Context.lookup_multiplicities")
        assert rep == {"lookups": total, "misses": 0, "first_miss": None}
        assert tuple(mult.shape) == (nc, n_sets, BINS) and str(mult.dtype) == "torch.int32"


@pytest.fixture(scope="module")
def one_block(pkg, ctx):
    """The histogram of one block of zero plaintext under the zero key, and of that key's slab alone (K = 12, N = 1: one block)."""
    out = {}
    for layout in mc.LAYOUTS:
        b = Batch(pkg, ctx, layout, 12, 1, [1], keys=np.zeros((1, 16), np.uint8), pt=np.zeros((1, 16), np.uint8))
        with_block, _ = b.expected()
        key_only, _ = Batch(pkg, ctx, layout, 12, 1, [0], keys=np.zeros((1, 16), np.uint8)).expected()
        out[layout] = (with_block[0, 0] - key_only[0, 0], key_only[0, 0])
    assert out[mc.DENSE][0][512] >= 16  # the first AddRoundKey alone: sixteen times 0 ^ 0
    return out


@pytest.mark.parametrize("k,n_sets,nc,per", mc.CONTENTION)
def test_identical_blocks_count_exactly(pkg, ctx, one_block, k, n_sets, nc, per):
    """Every block the same, so that all lanes add to the same few bins; at K = 23 bin 512 alone passes 65 535."""
    per = pkg.block_capacity(k, n_sets) if per is None else per
    cap0, capn = pkg.block_capacity(k, 1), (1 << k) // 1360
    first = [0 if s == 0 else cap0 + (s - 1) * capn for s in range(n_sets)]
    filled = [min(max(per - first[s], 0), cap0 if s == 0 else capn) for s in range(n_sets)]
    assert sum(filled) == per
    layout = mc.PACKED
    b = Batch(pkg, ctx, layout, k, n_sets, [per] * nc, keys=np.zeros((nc, 16), np.uint8), pt=np.zeros((nc * per, 16), np.uint8))
    block, key = one_block[layout]
    exp = np.stack([block * f + (key if s == 0 else 0) for s, f in enumerate(filled)])
    if (k, n_sets) == (23, 1):
        assert per == 6166 and exp[0, 512] > 65535
    for form in mc.FORMS:
        got, rep = b.count(G.DeviceArena(), form)
        same(got, np.broadcast_to(exp, got.shape), "form %d" % form)
        assert rep == {"lookups": nc * (400 + 1056 * per), "misses": 0, "first_miss": None}


def test_misses_are_counted_named_and_left_out_of_the_bins(pkg, ctx):
    import torch
    k, n_sets, counts, layout = 13, 3, [16, 3, 12], mc.PACKED
    b = Batch(pkg, ctx, layout, k, n_sets, counts, seed=77)
    clean, _ = b.expected()
    st = [pkg.column_stride(layout, i) for i in range(3)]
    kst = [pkg.key_column_stride(layout, i) for i in range(3)]
    py, pz, kpy = pkg.packed_index(1), pkg.packed_index(2), pkg.key_packed_index(1)
    tags, ktags = pkg.selector_tags()[:2]
    x_of = lambda blk, row: int(b.wit.x[blk * st[0] + row])  # noqa: E731
    # (tensor, byte index, unit, is key slab, row, (circuit, set, bin) that loses one)
    blk1 = int(b.offs[2]) + 5
    assert pkg.block_placement(k, n_sets, 5)[0] == 1 and tags[37] == 3
    sbox = (b.wit.y, blk1 * st[1] + int(py[37]), blk1, False, 37, (2, 1, 256 + x_of(blk1, 37)))
    last = b.n - 1
    assert tags[1347] == 2
    xor = (b.wit.z, last * st[2] + int(pz[1347]), last, False, 1347,
           (2, pkg.block_placement(k, n_sets, counts[2] - 1)[0], 512 + 256 * x_of(last, 1347) + int(b.wit.y[last * st[1] + int(py[1347])])))
    assert ktags[42] == 3
    key = (b.kw.ky, 1 * kst[1] + int(kpy[42]), 1, True, 42, (1, 0, 256 + int(b.kw.kx[1 * kst[0] + 42])))
    cases = [[sbox], [xor], [key], [sbox, key], [xor, sbox]]
    for case in cases:
        for t, at, *_ in case:
            t[at] ^= 0x40
        torch.cuda.synchronize()
        exp = clean.copy()
        for *_, where in case:
            exp[where] -= 1
        first = min((unit << 20 | int(is_key) << 19 | 1 << 16 | row, (unit, is_key, row)) for _t, _at, unit, is_key, row, _w in case)[1]
        for form in mc.FORMS:
            got, rep = b.count(G.DeviceArena(), form)
            same(got, exp, "form %d" % form)
            assert rep == {"lookups": 400 * 3 + 1056 * b.n, "misses": len(case), "first_miss": first}, (rep, first)
        model, misses = b.expected()  # the model, which reads the assembled columns, agrees
        same(model, exp, "model")
        assert misses == len(case)
        for t, at, *_ in case:
            t[at] ^= 0x40


# (K, N): K = 14 / N = 1 holds 10 blocks, K = 13 / N = 2 holds 4 + 6, so that a clamped circuit also crosses a set boundary
CLAMP_SHAPES = ((14, 1), (13, 2))
CLAMP_COUNTS = [3, 0, 10, 4, 0, 5]  # n = 22, the offsets 0 3 3 13 17 17 22; slab block 15 is block 2 of circuit 3
# offsets edited at {index: value}: none; a decreasing pair (circuit 2 counts nothing, circuit 3 from block 2 on: 10 of 15); a
# count of 14 above the capacity of 10 (blocks 13 ... 16 are counted by nobody); blocks 0 and 1 in front of offsets[0]; blocks 20
# and 21 behind offsets[C]; block 17 handed to the neighbouring circuit
CLAMP_EDITS = ({}, {3: 2}, {3: 3}, {0: 2}, {6: 20}, {4: 18, 5: 18})
CLAMPED_OUT = 2  # the edit of CLAMP_EDITS under which nobody counts slab block 15


def offsets_spec(pkg, k, n_sets, o, h, kh):
    """(hist int64[C, N, BINS], lookups) as include/aesw_mult.h words it: circuit c counts slab blocks o[c] + j for
    j < min(o[c+1] - o[c], capacity) when o[c+1] > o[c], and none otherwise; block j goes to the set Placement names for j; key
    slab c always counts into (c, 0)."""
    cap, nc = pkg.block_capacity(k, n_sets), len(o) - 1
    hist, blocks = np.zeros((nc, n_sets, BINS), np.int64), 0
    for c in range(nc):
        hist[c, 0] += kh[c]
        for j in range(min(o[c + 1] - o[c], cap) if o[c + 1] > o[c] else 0):
            hist[c, pkg.block_placement(k, n_sets, j)[0]] += h[o[c] + j]
            blocks += 1
    return hist, 400 * nc + 1056 * blocks


@pytest.mark.parametrize("layout", mc.LAYOUTS)
def test_offsets_are_clamped_as_the_header_says(pkg, ctx, layout):
    """Offsets that no valid counts make: "a count is clamped to aesw_block_capacity(k, n_sets), so the kernel reads only inside
    each circuit's own range" (include/aesw_mult.h), for both forms.  Every offset is at most n, so every block the specification
    names lies inside the slabs."""
    import torch
    for k, n_sets in CLAMP_SHAPES:
        cap = pkg.block_capacity(k, n_sets)
        assert cap == 10 and pkg.block_placement(k, n_sets, 9)[0] == n_sets - 1
        b = Batch(pkg, ctx, layout, k, n_sets, CLAMP_COUNTS, seed=k + layout)
        n, nc = b.n, b.nc
        assert n == 22 and b.offs.tolist() == [0, 3, 3, 13, 17, 17, 22]
        h, kh = b.parts()
        lists = []
        for edit in CLAMP_EDITS:
            o = [int(v) for v in b.offs]
            for at, value in edit.items():
                o[at] = value
            lists.append(o)
        rng = np.random.default_rng(1000 * k + layout)
        for i in range(40):  # anything at all inside [0, n], half of the lists sorted
            o = rng.integers(0, n + 1, nc + 1).tolist()
            lists.append(sorted(o) if i % 2 else o)
        assert any(o[c + 1] < o[c] for o in lists[:6] for c in range(nc)) and any(o[c + 1] - o[c] > cap for o in lists[:6] for c in range(nc))

        def count_all(o, miss=None):
            """Both forms under the offsets o; miss: None, or (report's first miss, (c, s, bin) one short) or () where nobody counts it"""
            assert len(o) == nc + 1 and all(0 <= v <= n for v in o), o  # nothing a kernel is told to read lies outside the slabs
            exp, lookups = offsets_spec(pkg, k, n_sets, o, h, kh)
            assert int(exp.max()) < min(G.CANARIES)  # no count holds a canary byte: one found in d_mult was left there
            want = {"lookups": lookups, "misses": 0, "first_miss": None}
            if miss:
                exp[miss[1]] -= 1
                want.update(misses=1, first_miss=miss[0])
            d_offs = torch.tensor(o, dtype=torch.int64, device="cuda")
            for canary, form in zip(G.CANARIES, mc.FORMS):
                got, rep = b.count(G.DeviceArena(canary), form, offsets=d_offs)  # the guards are checked in there
                same(got, exp, "offsets %s, form %d" % (o, form))
                assert rep == want, (o, form, rep, want)
                # no byte of d_mult is left as it was: an empty circuit's histograms are stored or zeroed too
                assert not (got.astype(np.uint32).view(np.uint8) == canary).any(), (o, form)

        for o in lists:
            count_all(o)

        # one miss: an S-box output of slab block 15 -- block 2 of circuit 3 as the batch is cut, set 0 in both shapes
        st = [pkg.column_stride(layout, i) for i in range(3)]
        row = 37
        assert pkg.selector_tags()[0][row] == 3 and pkg.block_placement(k, n_sets, 2)[0] == 0
        at = 15 * st[1] + (int(pkg.packed_index(1)[row]) if layout == mc.PACKED else row)
        lost = (3, 0, 256 + int(b.wit.x[15 * st[0] + row]))
        b.wit.y[at] ^= 0x40
        torch.cuda.synchronize()
        count_all(lists[0], miss=((15, False, row), lost))
        count_all(lists[CLAMPED_OUT], miss=())  # clamped out: nobody reads the cell
        b.wit.y[at] ^= 0x40
        torch.cuda.synchronize()


# K = 12 / N = 1024 / C = 4: 4 096 histograms, 1.09 GB of d_mult.  Zeroing them takes 66 561 workgroups of 1 024 16-byte stores; the
# DIRECT form launches 65 536 at most, so its zeroing loop takes a second trip.  5 and 7 blocks reach sets 0 ... 2 (1 + 3 + 3 blocks).
MANY = (12, 1024, [5, 0, 7, 1])


def test_more_histograms_than_the_zeroing_grid_has_workgroups(pkg, ctx):
    import torch
    k, n_sets, counts = MANY
    b = Batch(pkg, ctx, mc.PACKED, k, n_sets, counts, seed=4096)
    nc, words = b.nc, b.nc * n_sets * BINS
    assert nc * n_sets > 4033 and (words // 4 + 1023) // 1024 == 66561 > 65536
    h, kh = b.parts()
    exp = np.zeros((nc, 3, BINS), np.int64)
    for c in range(nc):
        exp[c, 0] += kh[c]
        for j in range(counts[c]):
            exp[c, pkg.block_placement(k, n_sets, j)[0]] += h[int(b.offs[c]) + j]  # sets 0 ... 2: IndexError otherwise
    assert exp[2, :, :].sum(axis=1).tolist() == [400 + 1056, 3 * 1056, 3 * 1056]
    arena = G.DeviceArena()
    mult = arena.out("mult", words * 4).view(torch.int32).view(nc, n_sets, BINS)  # the one large buffer, used by both forms in turn
    rep = arena.out("report", 24)
    word = int.from_bytes(bytes([arena.canary]) * 4, "little", signed=True)
    kept = []
    for form in mc.FORMS:
        assert arena.poisoned_on_device(mult) and arena.poisoned_on_device(rep)
        b.raw(mult, rep, form)
        arena.check_on_device()  # synchronises; the guard bands compared on the device
        assert not bool((mult == word).any()), "form %d left words of d_mult as they were" % form
        assert not bool(mult[:, 3:].any()), "form %d: a count in a set that holds no block" % form
        kept.append(mult[:, :3].clone())
        same(kept[-1].cpu().numpy().astype(np.int64), exp, "form %d" % form)
        assert pkg.api.mult_report_dict(rep.view(torch.int64)) == {"lookups": 400 * nc + 1056 * b.n, "misses": 0, "first_miss": None}
        arena.repoison()
    # equal everywhere: all zero from set 3 on, and the same in sets 0 ... 2
    assert torch.equal(kept[0], kept[1])


def test_a_captured_call_recounts_on_every_replay(pkg, ctx):
    import torch
    b = Batch(pkg, ctx, mc.PACKED, 13, 2, [6, 0, 7, 2], seed=14)
    exp, _ = b.expected()
    arena = G.DeviceArena()
    for form in mc.FORMS + (mc.FORM_AUTO,):
        mult, rep = b.outputs(arena, "_graph%d" % form)
        cap = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            b.raw(mult, rep, form)
        torch.cuda.synchronize()
        assert untouched(arena, mult, rep), "the captured call ran during capture"
        for i in range(3):
            graph.replay()
            torch.cuda.synchronize()
            same(mult.cpu().numpy().astype(np.int64), exp, "form %d, replay %d" % (form, i))  # no accumulation: nothing is poisoned again
            assert pkg.api.mult_report_dict(rep.view(torch.int64)) == {"lookups": 400 * 4 + 1056 * b.n, "misses": 0, "first_miss": None}
    arena.check()


def test_refusals_leave_the_outputs_alone_and_say_why(pkg, ctx):
    import torch
    b = Batch(pkg, ctx, mc.PACKED, 12, 1, [1], seed=3)
    arena = G.DeviceArena()
    mult, rep = b.outputs(arena)
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    assert b.raw(mult, rep, mc.FORM_AUTO, layout=mc.VALUES, expect=1) == 1 and "aesw_mult_count_device" in err() and "VALUES" in err()
    for k in (1, 31):
        assert b.raw(mult, rep, mc.FORM_AUTO, k=k, expect=1) == 1 and "k must be" in err()
    flat = mult.view(-1)
    assert b.raw(flat[1:], rep, mc.FORM_AUTO, expect=1) == 1 and "d_mult" in err()  # 4-byte aligned only
    assert b.raw(mult, rep, 3, expect=1) == 1 and "form" in err()
    torch.cuda.synchronize()
    assert untouched(arena, mult, rep)
    arena.check()
    with pytest.raises(pkg.AeswError) as e:
        ctx.lookup_multiplicities(12, 1, b.wit, b.kw, [1], layout=mc.VALUES)
    assert e.value.status == pkg.api.ERR_INVALID_ARG
    group = pkg.Group([0])
    try:
        with pytest.raises(pkg.AeswError) as e:
            group.lookup_multiplicities(12, 1, b.wit, b.kw, [1])
        assert e.value.status == pkg.api.ERR_INVALID_ARG
        lib = pkg.api.load_mult_library()
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in b.kw[:4]])
        rc = lib.aesw_mult_count_device(group._h, 12, 1, 1, b.d_offs.data_ptr(), mc.PACKED, b.wit.x.data_ptr(), b.wit.y.data_ptr(),
                                        b.wit.z.data_ptr(), C.byref(ks), mult.data_ptr(), rep.data_ptr(), ctx._stream())
        assert rc == 1 and "aesw_mult_count_device" in group._lib.aesw_last_error(group._h).decode()
    finally:
        group.close()
    torch.cuda.synchronize()
    assert untouched(arena, mult, rep)
