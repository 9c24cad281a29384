"""Many circuits per launch (aesw_assemble_advice_circuits_device and Context.circuits) on the GPU, every output a poisoned,
guard-banded view (tests/guarded.py) whose guards are checked.

Expected values: the CPU oracle per circuit -- its blocks encrypted under its key repeated per block, its key slab, and
every advice cell of oracle.circuit(k, n_sets, key_c, pts_c) -- and, cell for cell, the one-circuit entry point
aesw_assemble_advice_device on the same slabs.  The case list is tests/circuit_cases.py."""
import ctypes as C

import numpy as np
import pytest

import circuit_cases as cc
import guarded as G
import oracle_lib as ol

pytestmark = pytest.mark.gpu

PACKED = ol.PACKED


def _context(pkg, xt):
    tables = None if xt else G.random_tables()
    c = pkg.Context(0, tables=tables)
    assert c.uses_xtime_path == xt
    return c, ol.Oracle(tables=tables)


def _fr_lut():
    from test_gpu_round4 import _fr_lut as lut
    return lut()


def _expected_advice(orc, k, n_sets, key, pts):
    """The advice matrix [3N+1, 2^K] of one circuit: the restated synthesize() where the reference runs (K >= 11), the clipped
    key slab below (no block fits there)."""
    if k >= 11:
        with orc.circuit(k, n_sets, key, pts, record_copies=False) as circ:
            return np.stack([circ.advice(col) for col in range(3 * n_sets + 1)])
    assert len(pts) == 0
    from test_gpu_round4 import _small_k_expectation
    return _small_k_expectation(orc, k, n_sets, key)


def _run(pkg, ctx, arena, k, n_sets, keys, pt, counts):
    """Key schedule, the blocks' witness (per-block keys: each block under its circuit's key) and both assemble forms of every
    circuit into guarded outputs of `arena`."""
    nc, n, ncol, rows = len(counts), len(pt), 3 * n_sets + 1, 1 << k
    dkeys = arena.input("keys", keys)
    kw = arena.key_witness(pkg, nc, PACKED, want_rk=True)
    G.key_schedule(ctx, dkeys, PACKED, kw)
    wit = arena.witness(pkg, max(n, 1), PACKED, want_ct=True, key_slab=False)  # n = 0: key rows only, no block is read
    if n:
        ctx.encrypt_witness(arena.input("pt", pt), arena.input("keys_per_block", np.repeat(keys, counts, axis=0)), layout=PACKED, out=wit)
    adv_b = arena.out("advice_bytes", nc * ncol * rows, (nc, ncol, rows))
    adv_f = arena.out("advice_fr", nc * ncol * rows * 32, (nc, ncol, rows, 32))
    assert arena.poisoned(adv_b) and arena.poisoned(adv_f)
    ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=False, n_blocks=n, out=adv_b)
    ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=True, n_blocks=n, out=adv_f)
    return kw, wit, adv_b, adv_f


@pytest.mark.parametrize("path", cc.TABLE_PATHS)
@pytest.mark.parametrize("k,n_sets,nc", cc.SHAPES, ids=["k%d-n%d-c%d" % s for s in cc.SHAPES])
def test_circuits_match_the_oracle_and_the_one_circuit_path(pkg, k, n_sets, nc, path):
    import torch
    ctx, orc = _context(pkg, path == "xtime")
    try:
        rng = np.random.default_rng(k * 1000 + n_sets * 100 + nc)
        cap = pkg.block_capacity(k, n_sets)
        rows = 1 << k
        cap0 = (rows - 1760) // 1360 if rows >= 1760 else 0
        counts = cc.ragged_counts(cap, cap0, n_sets, nc, rng)
        n = sum(counts)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        keys = rng.integers(0, 256, (nc, 16), dtype=np.uint8)
        pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        if n > 1:
            pt[1], keys[np.searchsorted(offs, 1, side="right") - 1] = 0xFF, 0  # S_BOX[255] in the first round
        arena = G.DeviceArena(G.CANARIES[(k + nc) % 2])
        kw, wit, adv_b, adv_f = _run(pkg, ctx, arena, k, n_sets, keys, pt, counts)
        arena.check()

        # key slabs and round keys: the oracle's schedule of the C keys
        okw = orc.key_schedule_witness(keys, layout=PACKED)
        for name in ("w", "kx", "ky", "kz", "rk"):
            G.assert_bytes("key slab %s" % name, getattr(kw, name).cpu().numpy(), getattr(okw, name))
        # block slabs and ciphertexts: every block under its circuit's key
        if n:
            ow = orc.encrypt_witness(pt, np.repeat(keys, counts, axis=0), layout=PACKED)
            for name in "xyz":
                G.assert_bytes("column %s" % name, getattr(wit, name).cpu().numpy(), getattr(ow, name))
            G.assert_bytes("ct", wit.ct.cpu().numpy(), ow.ct)
        # advice: every cell of every circuit, bytes against the oracle, Fr against the bytes through Fp::from
        got_b = adv_b.cpu().numpy()
        for c in range(nc):
            exp = _expected_advice(orc, k, n_sets, keys[c], pt[offs[c]:offs[c + 1]])
            G.assert_bytes("advice of circuit %d (%d blocks)" % (c, counts[c]), got_b[c], exp)
        lut = torch.from_numpy(_fr_lut()).cuda()
        assert torch.equal(adv_f, lut[adv_b.long()]), "Fr advice differs from Fp::from(byte advice)"

        # the one-circuit entry point on the same slabs, circuit by circuit
        single = G.DeviceArena(G.CANARIES[(k + nc + 1) % 2])
        strides = [pkg.column_stride(PACKED, i) for i in range(3)]
        kstrides = [96] + [pkg.key_column_stride(PACKED, i) for i in range(3)]
        ncol = 3 * n_sets + 1
        for c in range(nc):
            lo, hi = int(offs[c]), int(offs[c + 1])
            w1 = pkg.Witness(*[wit[i][lo * strides[i]:hi * strides[i]] for i in range(3)], None, None)
            k1 = pkg.KeyWitness(*[kw[i][c * kstrides[i]:(c + 1) * kstrides[i]] for i in range(4)], None)
            for as_fr, whole in ((False, adv_b), (True, adv_f)):
                shape = (ncol, rows, 32) if as_fr else (ncol, rows)
                out = single.out("single_%d_%d" % (c, as_fr), int(np.prod(shape)), shape)
                ctx.assemble_advice(k, n_sets, w1, k1, hi - lo, layout=PACKED, as_fr=as_fr, out=out)
                assert torch.equal(out, whole[c]), "circuit %d (as_fr %s) differs from aesw_assemble_advice_device" % (c, as_fr)
        single.check()
    finally:
        ctx.close()


def test_three_launches_captured_into_one_graph(pkg, oracle):
    """Key schedule + encrypt + circuit assemble for C = 5 circuits captured into one hipGraph and replayed once: the
    outputs, poisoned before the replay, equal the same calls made eagerly."""
    import torch
    k, n_sets = 14, 3
    counts = [34, 0, 7, 34, 11]
    n, nc = sum(counts), len(counts)
    rng = np.random.default_rng(14)
    keys = rng.integers(0, 256, (nc, 16), dtype=np.uint8)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ctx = pkg.Context(0)
    try:
        eager = G.DeviceArena(G.CANARIES[0])
        kw_e, wit_e, adv_e, fr_e = _run(pkg, ctx, eager, k, n_sets, keys, pt, counts)
        eager.check()

        arena = G.DeviceArena(G.CANARIES[1])
        dkeys, dpt = arena.input("keys", keys), arena.input("pt", pt)
        dkpb = arena.input("keys_per_block", np.repeat(keys, counts, axis=0))
        kw = arena.key_witness(pkg, nc, PACKED, want_rk=True)
        wit = arena.witness(pkg, n, PACKED, want_ct=True, key_slab=False)
        ncol, rows = 3 * n_sets + 1, 1 << k
        adv = arena.out("advice_fr", nc * ncol * rows * 32, (nc, ncol, rows, 32))
        d_offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, counts, n).view(np.int64)).cuda()
        torch.cuda.synchronize()
        cap = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            G.key_schedule(ctx, dkeys, PACKED, kw)
            ctx.encrypt_witness(dpt, dkpb, layout=PACKED, out=wit)
            ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=True, out=adv, _offsets=d_offs)
        torch.cuda.synchronize()
        assert arena.poisoned(adv) and arena.poisoned(wit.y), "a captured call ran during capture"
        graph.replay()
        torch.cuda.synchronize()
        arena.check()
        for name in ("w", "kx", "ky", "kz", "rk"):
            assert torch.equal(getattr(kw, name), getattr(kw_e, name)), name
        for name in ("x", "y", "z", "ct"):
            assert torch.equal(getattr(wit, name), getattr(wit_e, name)), name
        assert torch.equal(adv, fr_e)
        ow = oracle.encrypt_witness(pt, np.repeat(keys, counts, axis=0), layout=PACKED)
        G.assert_bytes("replayed y", wit.y.cpu().numpy(), ow.y)
    finally:
        ctx.close()


def test_context_circuits_one_call(pkg, oracle):
    """Context.circuits: three launches on one stream, advice shaped [C, 3N+1, 2^K(, 32)]."""
    import torch
    k, n_sets, counts = 12, 1, [1, 0, 1]
    rng = np.random.default_rng(12)
    keys = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    pt = rng.integers(0, 256, (2, 16), dtype=np.uint8)
    with pkg.Context(0) as ctx:
        dkeys, dpt = torch.from_numpy(keys).cuda(), torch.from_numpy(pt).cuda()
        wit, kw, byte = ctx.circuits(k, n_sets, dkeys, dpt, counts, as_fr=False)
        _w, _k, fr = ctx.circuits(k, n_sets, dkeys, dpt, counts, as_fr=True)
        torch.cuda.synchronize()
        assert tuple(byte.shape) == (3, 4, 1 << k) and tuple(fr.shape) == (3, 4, 1 << k, 32)
        offs = np.cumsum([0] + counts)
        exp = np.stack([_expected_advice(oracle, k, n_sets, keys[c], pt[offs[c]:offs[c + 1]]) for c in range(3)])
        G.assert_bytes("Context.circuits advice", byte.cpu().numpy(), exp)
        G.assert_bytes("Context.circuits Fr advice", fr.cpu().numpy(), _fr_lut()[exp])
        G.assert_bytes("Context.circuits ct", wit.ct.cpu().numpy(), oracle.encrypt_witness(pt, np.repeat(keys, counts, axis=0)).ct)
        G.assert_bytes("Context.circuits key slab", kw.kx.cpu().numpy(), oracle.key_schedule_witness(keys).kx)


def test_group_refuses_the_circuit_calls(pkg):
    import torch
    g = pkg.Group([0])
    try:
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        p = buf.data_ptr()
        lib = g._lib
        ks = pkg.api.KeySlab(p, p, p, p)
        rc = lib.aesw_assemble_advice_circuits_device(g._h, 14, 1, 1, p, PACKED, p, p, p, C.byref(ks), 1, p, None)
        assert rc == 1, rc  # AESW_ERR_INVALID_ARG
        for name in ("assemble_advice_circuits", "circuits"):
            with pytest.raises(pkg.AeswError):
                getattr(g, name)()
    finally:
        g.close()
