"""libaesw_ntt.so on the GPU against tests/ntt_model.py, every written cell, on poisoned, guard-banded buffers.

nc.SHAPES: k = 10 (one pass) and NTT_PASS_LOG + 1 = 11 (a second pass of one stage, three columns, so grid.y and the column stride
matter); two full passes and three passes are above what a model run follows and are tests/test_gpu_ntt_reach.py's.  All four
transforms, both zeta_sel and ext_k - k in {0, 1, 3} (nc.EXTENDED); coeff_to_extended also as evaluate(coeff, zeta * omega_ext^j)
at the first, the last and 64 seeded rows; the same-size calls in place and out of place; the three fr_store_modes; round trips on
the device; tables built for max_k = 20 at k = 10 and 17; every refusal; an input that is not canonical."""
import functools

import numpy as np
import pytest

import guarded as G
import ntt_cases as nc
import ntt_model as nm

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def column(rows, seed):
    return tuple(nm.seeded_values(rows, seed))


@functools.lru_cache(maxsize=None)
def expected(name, k, ext_k, sel, seed):
    """(input cells, output cells) of one column, uint8 [rows, 32]"""
    rows = 1 << (ext_k if name == "extended_to_coeff" else k)
    values = list(column(rows, seed))
    out = {"coeff_to_lagrange": lambda: nm.coeff_to_lagrange(values, k), "lagrange_to_coeff": lambda: nm.lagrange_to_coeff(values, k),
           "coeff_to_extended": lambda: nm.coeff_to_extended(values, k, ext_k, sel), "extended_to_coeff": lambda: nm.extended_to_coeff(values, ext_k, sel)}[name]()
    return nm.to_cells(values), nm.to_cells(out)


def world(name, k, ext_k, sel, n_cols, seed):
    pairs = [expected(name, k, ext_k, sel, seed + c) for c in range(n_cols)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def put(arena, name, cells):
    """a guarded, 16-byte aligned device copy of uint8 cells"""
    import torch
    t = arena.out(name, cells.size, cells.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(cells)).to(t.device))
    return t


@functools.lru_cache(maxsize=None)
def tables_for(ctx, max_k):
    return ctx.ntt_tables(max_k)


def run(ctx, arena, name, k, ext_k, sel, d_in, tables, in_place=False):
    n_cols = d_in.shape[0]
    rows = 1 << (k if name in ("coeff_to_lagrange", "lagrange_to_coeff") else ext_k)
    out = d_in if in_place else arena.out("out", n_cols * rows * 32, (n_cols, rows, 32))
    if name in ("coeff_to_lagrange", "lagrange_to_coeff"):
        return getattr(ctx, name)(d_in, k, tables, out=out)
    if name == "coeff_to_extended":
        return ctx.coeff_to_extended(d_in, k, ext_k, tables, zeta_sel=sel, out=out)
    return ctx.extended_to_coeff(d_in, ext_k, tables, zeta_sel=sel, out=out)


@pytest.mark.parametrize("name", ("coeff_to_lagrange", "lagrange_to_coeff"))
@pytest.mark.parametrize("shape", nc.SHAPES, ids=lambda s: "k%d-c%d" % s)
def test_the_same_size_transforms_are_the_models_in_place_and_out_of_place(ctx, name, shape):
    k, n_cols = shape
    cells, exp = world(name, k, k, 0, n_cols, 0x7361 + k)
    tables = tables_for(ctx, k)
    for in_place in (False, True):
        arena = G.DeviceArena(G.CANARIES[in_place])
        d_in = put(arena, "in", cells)
        got = run(ctx, arena, name, k, k, 0, d_in, tables, in_place)
        arena.check()
        G.assert_bytes("%s k=%d in_place=%s" % (name, k, in_place), got.cpu().numpy(), exp)
        if not in_place:
            G.assert_bytes("the input is left alone", d_in.cpu().numpy(), cells)


@pytest.mark.parametrize("case", nc.EXTENDED, ids=lambda c: "k%d-e%d-z%d-c%d" % c)
def test_the_extended_transforms_are_the_models_and_the_evaluations_on_the_coset(ctx, case):
    k, ext_k, sel, n_cols = case
    tables = tables_for(ctx, ext_k)
    cells, exp = world("coeff_to_extended", k, ext_k, sel, n_cols, 0x6578 + ext_k)
    arena = G.DeviceArena(G.CANARIES[sel])
    d_in = put(arena, "coeff", cells)
    ext = run(ctx, arena, "coeff_to_extended", k, ext_k, sel, d_in, tables)
    arena.check()
    G.assert_bytes("coeff_to_extended %r" % (case,), ext.cpu().numpy(), exp)
    rng = np.random.default_rng(0x6576 + ext_k)
    rows = [0, (1 << ext_k) - 1] + [int(v) for v in rng.integers(0, 1 << ext_k, 64)]
    coeff = list(column(1 << k, 0x6578 + ext_k + n_cols - 1))  # the last column
    got = nm.from_cells(ext[n_cols - 1].cpu().numpy()[rows])
    w = nm.omega(ext_k)
    assert got == [nm.evaluate(coeff, nm.ZETAS[sel] * pow(w, j, nm.R) % nm.R) for j in rows]
    # and back: the coefficients followed by zeros, out of place and in place
    back = run(ctx, arena, "extended_to_coeff", k, ext_k, sel, ext, tables)
    arena.check()
    padded = np.concatenate([cells, np.zeros((n_cols, (1 << ext_k) - (1 << k), 32), np.uint8)], axis=1)
    G.assert_bytes("extended_to_coeff %r" % (case,), back.cpu().numpy(), padded)
    again = run(ctx, arena, "extended_to_coeff", k, ext_k, sel, ext, tables, in_place=True)
    arena.check()
    G.assert_bytes("extended_to_coeff in place %r" % (case,), again.cpu().numpy(), padded)


def test_extended_to_coeff_of_a_dense_column_is_the_models(ctx):
    k, ext_k, sel, n_cols = 10, 11, 0, 2
    cells, exp = world("extended_to_coeff", k, ext_k, sel, n_cols, 0x6532)
    arena = G.DeviceArena()
    got = run(ctx, arena, "extended_to_coeff", k, ext_k, sel, put(arena, "ext", cells), tables_for(ctx, ext_k))
    arena.check()
    G.assert_bytes("extended_to_coeff dense", got.cpu().numpy(), exp)


@pytest.mark.parametrize("mode", nc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(ctx, mode):
    k, n_cols = nc.SHAPES[1]
    cells, exp = world("lagrange_to_coeff", k, k, 0, n_cols, 0x7361 + k)
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[mode % 2])
        got = run(ctx, arena, "lagrange_to_coeff", k, k, 0, put(arena, "in", cells), tables_for(ctx, k))
        arena.check()
    finally:
        ctx.set_option("fr_store_mode", before)
    G.assert_bytes("mode %d" % mode, got.cpu().numpy(), exp)


@pytest.mark.parametrize("k", nc.TABLES_KS)
def test_tables_of_a_larger_max_k_serve_a_smaller_transform(ctx, k):
    import torch
    arena = G.DeviceArena()
    need = int(ctx_lib(ctx).aesw_ntt_tables_bytes(nc.TABLES_MAX_K))
    tables = ctx.ntt_tables(nc.TABLES_MAX_K, _out=arena.out("tables", need, (need // 32, 32)))
    cells, exp = world("coeff_to_lagrange", k, k, 0, 1, 0x746b + k)
    d_in = put(arena, "in", cells)
    got = run(ctx, arena, "coeff_to_lagrange", k, k, 0, d_in, tables)
    arena.check()
    G.assert_bytes("max_k %d at k %d" % (nc.TABLES_MAX_K, k), got.cpu().numpy(), exp)
    # the round trip on the device, bit for bit, in place
    back = run(ctx, arena, "lagrange_to_coeff", k, k, 0, got, tables, in_place=True)
    arena.check()
    assert torch.equal(back, d_in)


def ctx_lib(ctx):
    import __graft_entry__ as ge
    return ge.load_package().api.load_ntt_library()


def test_the_round_trips_on_the_device_give_the_input_back(ctx):
    import torch
    k, ext_k, n_cols = 11, 13, 3
    tables = tables_for(ctx, ext_k)
    cells, _ = world("coeff_to_lagrange", k, k, 0, n_cols, 0x7274)
    arena = G.DeviceArena(G.CANARIES[1])
    d_in = put(arena, "in", cells)
    there = run(ctx, arena, "coeff_to_lagrange", k, k, 0, d_in, tables)
    assert torch.equal(run(ctx, arena, "lagrange_to_coeff", k, k, 0, there, tables), d_in)
    for sel in (0, 1):
        ext = run(ctx, arena, "coeff_to_extended", k, ext_k, sel, d_in, tables)
        back = run(ctx, arena, "extended_to_coeff", k, ext_k, sel, ext, tables)
        assert torch.equal(back[:, :1 << k], d_in) and not back[:, 1 << k:].any()
    arena.check()


def test_an_input_that_is_not_canonical_leaves_the_guard_bands_whole(ctx):
    k, ext_k, n_cols = 11, 12, 2
    tables = tables_for(ctx, ext_k)
    ones = np.full((n_cols, 1 << k, 32), 0xFF, np.uint8)
    arena = G.DeviceArena()
    d_in = put(arena, "in", ones)
    outs = [run(ctx, arena, "coeff_to_lagrange", k, k, 0, d_in, tables), run(ctx, arena, "lagrange_to_coeff", k, k, 0, d_in, tables),
            run(ctx, arena, "coeff_to_extended", k, ext_k, 1, d_in, tables)]
    outs.append(run(ctx, arena, "extended_to_coeff", k, ext_k, 1, outs[2], tables))
    arena.check()
    G.assert_bytes("the input is left alone", d_in.cpu().numpy(), ones)
    for o in outs:  # every cell was written: no run of eight canary bytes is left (a cell of canaries is not canonical and not likely)
        assert not (o.cpu().numpy().reshape(-1, 8) == arena.canary).all(axis=1).any()


def test_every_refusal_leaves_the_poison_whole(pkg, ctx):
    import torch
    lib, api = pkg.api.load_ntt_library(), pkg.api
    k, ext_k, n_cols = 11, 12, 2
    arena = G.DeviceArena()
    tables = tables_for(ctx, 12)
    d_in = put(arena, "in", world("coeff_to_lagrange", k, k, 0, n_cols, 0x7266)[0])
    out = arena.out("out", n_cols * (32 << ext_k))
    ws = arena.out("ws", n_cols * (32 << ext_k))
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    i, o, t, w = d_in.data_ptr(), out.data_ptr(), tables.data_ptr(), ws.data_ptr()
    same = lambda f, *a: getattr(lib, "aesw_ntt_%s_device" % f)(ctx._h, *a, s)  # noqa: E731
    refusals = [
        ("lagrange_to_coeff", (9, n_cols, i, o, t, 12, w), "k"), ("lagrange_to_coeff", (29, n_cols, i, o, t, 28, w), "k"),
        ("coeff_to_lagrange", (k, 0, i, o, t, 12, w), "n_cols"), ("coeff_to_lagrange", (k, 65536, i, o, t, 12, w), "n_cols"),
        ("coeff_to_lagrange", (k, n_cols, i, o, t, 10, w), "max_k"), ("coeff_to_lagrange", (k, n_cols, i, o, t, 29, w), "max_k"),
        ("lagrange_to_coeff", (k, n_cols, None, o, t, 12, w), "input"), ("lagrange_to_coeff", (k, n_cols, i, None, t, 12, w), "output"),
        ("lagrange_to_coeff", (k, n_cols, i + 8, o, t, 12, w), "aligned"), ("lagrange_to_coeff", (k, n_cols, i, o + 4, t, 12, w), "aligned"),
        ("lagrange_to_coeff", (k, n_cols, i, o, None, 12, w), "d_tables"), ("lagrange_to_coeff", (k, n_cols, i, o, t + 8, 12, w), "d_tables"),
        ("lagrange_to_coeff", (k, n_cols, i, o, t, 12, w + 8), "d_workspace"),
        ("lagrange_to_coeff", (k, n_cols, o, o, t, 12, None), "d_workspace"),          # in place, two passes, no workspace
        ("lagrange_to_coeff", (k, n_cols, o, o, t, 12, o + 64), "d_workspace"),        # the workspace overlaps the columns
        ("coeff_to_lagrange", (k, n_cols, o + 32, o, t, 12, w), "overlap"),            # a partial overlap
        ("coeff_to_lagrange", (k, n_cols, i, o, o + 64, 12, w), "d_tables"),           # the tables lie in the output
        ("coeff_to_extended", (k, ext_k, 2, n_cols, i, o, t, 12, w), "zeta_sel"), ("coeff_to_extended", (k, 10, 1, n_cols, i, o, t, 12, w), "ext_k"),
        ("coeff_to_extended", (k, 13, 1, n_cols, i, o, t, 12, w), "max_k"), ("coeff_to_extended", (k, ext_k, 1, n_cols, o, o, t, 12, w), "overlap"),
        ("coeff_to_extended", (k, ext_k, 1, n_cols, o + 32, o, t, 12, w), "overlap"),
        ("extended_to_coeff", (ext_k, 2, n_cols, i, o, t, 12, w), "zeta_sel"), ("extended_to_coeff", (9, 1, n_cols, i, o, t, 12, w), "k"),
    ]
    for f, args, word in refusals:
        assert same(f, *args) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_ntt_%s_device" % f) in err() and word in err(), (f, args, err())
    assert lib.aesw_ntt_tables_device(ctx._h, 9, o, s) == api.ERR_INVALID_ARG and "max_k" in err()
    assert lib.aesw_ntt_tables_device(ctx._h, 12, None, s) == api.ERR_INVALID_ARG and lib.aesw_ntt_tables_device(ctx._h, 12, o + 8, s) == api.ERR_INVALID_ARG
    assert lib.aesw_ntt_lagrange_to_coeff_device(None, k, n_cols, i, o, t, 12, w, s) == api.ERR_INVALID_ARG
    torch.cuda.synchronize()
    arena.check()
    assert arena.poisoned_on_device(out) and arena.poisoned_on_device(ws)
    # the Python face says the same before it calls
    with pytest.raises(pkg.AeswError):
        ctx.ntt_tables(9)
    with pytest.raises(pkg.AeswError):
        ctx.coeff_to_extended(d_in, k, 10, tables)
    with pytest.raises(ValueError):
        ctx.lagrange_to_coeff(d_in, 12, tables)
    with pytest.raises(ValueError):
        ctx.coeff_to_extended(d_in, k, 13, tables)  # tables of max_k 12
    with pytest.raises(pkg.AeswError):
        ctx.coeff_to_extended(d_in, k, ext_k, tables, zeta_sel=2, out=out.view(n_cols, 1 << ext_k, 32))
    assert arena.poisoned_on_device(out)
