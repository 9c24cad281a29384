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

    def raw(self, mult, report, form, key_slabs=True, layout=None, k=None, expect=0):
        """The test-facing C entry point on torch's current stream; returns the status."""
        lib, ctx = self.pkg.api.load_mult_library(), self.ctx
        ks = self.pkg.api.KeySlab(*[t.data_ptr() for t in self.kw[:4]])
        rc = lib.aesw_mult_count_device_form(
            ctx._h, self.k if k is None else k, self.n_sets, self.nc, self.d_offs.data_ptr(), self.layout if layout is None else layout,
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
