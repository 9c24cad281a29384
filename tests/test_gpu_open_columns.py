"""libaesw_open.so on the GPU against tests/open_model.py, every written cell, on poisoned, guard-banded buffers.

oc.SHAPES: k = 10, one column, one point (one chunk) and k = 11, three columns, three points (a carry across two chunks; grid.y,
the column stride and the point stride matter); the second turn of the carry is tests/test_gpu_open_reach.py's.  The points of
oc.points: 0, 1, omega_k, r - 1 and two seeded values.  The columns: seeded, all zero, and only the top coefficient set.  Divide out
of place and in place; fold without an accumulator, with one of its own and with one in place, and two folds of 2 + 1 columns
against one of 3; the quotient evaluated at a second point against p(y) - p(z) == q(y) (y - z), on the device; the three
fr_store_modes; an input that is not canonical; every refusal."""
import functools

import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import open_cases as oc
import open_model as om

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def columns(k, n_cols):
    """n_cols columns as plain values: seeded ones, the last but one all zero and the last only its top coefficient (where there are three)"""
    cols = [nm.seeded_values(1 << k, 0x6f63 + 8 * k + c) for c in range(n_cols)]
    if n_cols >= 3:
        cols[-2] = [0] * (1 << k)
        cols[-1] = [0] * ((1 << k) - 1) + [cols[-1][-1]]
    return tuple(tuple(c) for c in cols)


@functools.lru_cache(maxsize=None)
def coeff_cells(k, n_cols):
    return np.stack([nm.to_cells(c) for c in columns(k, n_cols)])


@functools.lru_cache(maxsize=None)
def divided(k, n_cols, z):
    """(quotient cells [n_cols, 2^k, 32], remainder cells [n_cols, 32]) by the model, once per point"""
    pairs = [om.divide(list(c), z) for c in columns(k, n_cols)]
    return np.stack([nm.to_cells(q) for q, _rem in pairs]), nm.to_cells([rem for _q, rem in pairs])


def put(arena, name, cells):
    """a guarded, 16-byte aligned device copy of uint8 cells"""
    import torch
    t = arena.out(name, cells.size, cells.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(cells)).to(t.device))
    return t


def point_sets(k, n_points, seed):
    """oc.points in groups of n_points, the last group filled up from the front"""
    pts = oc.points(k, seed)
    return [(pts[i:i + n_points] + pts)[:n_points] for i in range(0, len(pts), n_points)]


def workspace(pkg, arena, k, n_cols, n_points):
    return arena.out("ws", int(pkg.api.load_open_library().aesw_open_workspace_bytes(k, n_cols, n_points)))


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "k%d-c%d-p%d" % s)
def test_evaluate_is_the_model_at_every_point(pkg, ctx, shape):
    k, n_cols, n_points = shape
    cells = coeff_cells(k, n_cols)
    for i, pts in enumerate(point_sets(k, n_points, 0x7074 + k)):
        arena = G.DeviceArena(G.CANARIES[i % 2])
        d_coeff = put(arena, "coeff", cells)
        d_points = put(arena, "points", nm.to_cells(pts))
        got = ctx.evaluate_columns(d_coeff, k, d_points, out=arena.out("evals", n_cols * n_points * 32, (n_cols, n_points, 32)),
                                   _workspace=workspace(pkg, arena, k, n_cols, n_points))
        arena.check()
        exp = nm.to_cells([om.evaluate(c, z) for c in columns(k, n_cols) for z in pts]).reshape(n_cols, n_points, 32)
        G.assert_bytes("evaluate %r at %r" % (shape, pts), got.cpu().numpy(), exp)
        G.assert_bytes("the columns are left alone", d_coeff.cpu().numpy(), cells)
        G.assert_bytes("the points are left alone", d_points.cpu().numpy(), nm.to_cells(pts))


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "k%d-c%d-p%d" % s)
def test_divide_is_the_model_in_place_and_out_of_place(pkg, ctx, shape):
    k, n_cols, _n_points = shape
    cells = coeff_cells(k, n_cols)
    for i, z in enumerate(oc.points(k, 0x7074 + k)):
        exp_q, exp_rem = divided(k, n_cols, z)
        for in_place in ((False, True) if i % 2 == 0 else (True, False)):
            arena = G.DeviceArena(G.CANARIES[(i + in_place) % 2])
            d_coeff = put(arena, "coeff", cells)
            out = d_coeff if in_place else arena.out("quot", cells.size, cells.shape)
            quot, rem = ctx.divide_columns(d_coeff, k, put(arena, "point", nm.to_cells([z])), out=out, _rem=arena.out("rem", n_cols * 32, (n_cols, 32)),
                                           _workspace=workspace(pkg, arena, k, n_cols, 1))
            arena.check()
            G.assert_bytes("divide %r at %d in_place=%s" % (shape, z, in_place), quot.cpu().numpy(), exp_q)
            G.assert_bytes("the remainder %r at %d in_place=%s" % (shape, z, in_place), rem.cpu().numpy(), exp_rem)
            if not in_place:
                G.assert_bytes("the input is left alone", d_coeff.cpu().numpy(), cells)
    # only the top coefficient set: q[2^k - 2] = c_top, q[2^k - 1] = 0, rem = c_top z^(2^k - 1) -- the model's figures, in closed form
    if n_cols >= 3:
        top = columns(k, n_cols)[-1][-1]
        q = nm.from_cells(exp_q[-1])
        assert q[-2] == top and q[-1] == 0 and nm.from_cells(exp_rem[-1]) == [top * pow(z, (1 << k) - 1, nm.R) % nm.R]
        assert not exp_q[-2].any() and not exp_rem[-2].any()  # the zero column


def test_fold_is_the_model_with_and_without_an_accumulator_and_in_place(ctx):
    import torch
    k, n_cols, _ = oc.SHAPES[1]
    cols = [list(c) for c in columns(k, n_cols)]
    cells = coeff_cells(k, n_cols)
    acc = nm.seeded_values(1 << k, 0x6163)
    for i, v in enumerate(oc.points(k, 0x76)):
        arena = G.DeviceArena(G.CANARIES[i % 2])
        d_coeff, d_v, d_acc = put(arena, "coeff", cells), put(arena, "v", nm.to_cells([v])), put(arena, "acc", nm.to_cells(acc))
        new = lambda: arena.out("folded", 32 << k, (1 << k, 32))  # noqa: E731
        bare = ctx.fold_columns(d_coeff, k, d_v.view(32), out=new())
        separate = ctx.fold_columns(d_coeff, k, d_v.view(32), acc=d_acc, out=new())
        # two successive folds of 2 + 1 columns, the second into its own accumulator, are one fold of 3
        first = ctx.fold_columns(d_coeff[:2], k, d_v.view(32), acc=d_acc, out=new())
        second = ctx.fold_columns(d_coeff[2:], k, d_v.view(32), acc=first, out=first)
        arena.check()
        assert second.data_ptr() == first.data_ptr()
        G.assert_bytes("fold without acc, v=%d" % v, bare.cpu().numpy(), nm.to_cells(om.fold(cols, v)))
        G.assert_bytes("fold with acc, v=%d" % v, separate.cpu().numpy(), nm.to_cells(om.fold(cols, v, acc)))
        assert torch.equal(second, separate)
        G.assert_bytes("the accumulator is left alone", d_acc.cpu().numpy(), nm.to_cells(acc))
        G.assert_bytes("the columns are left alone", d_coeff.cpu().numpy(), cells)
    # one column of k = 10, the other shape
    k1 = oc.SHAPES[0][0]
    arena = G.DeviceArena()
    one = ctx.fold_columns(put(arena, "coeff", coeff_cells(k1, 1)), k1, v, out=arena.out("folded", 32 << k1, (1 << k1, 32)))
    arena.check()
    G.assert_bytes("one column", one.cpu().numpy(), coeff_cells(k1, 1)[0])


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "k%d-c%d-p%d" % s)
def test_the_quotient_at_a_second_point_satisfies_the_identity_on_the_device(pkg, ctx, shape):
    k, n_cols, _ = shape
    z, y = nm.seeded_values(2, 0x6964 + k)
    arena = G.DeviceArena()
    d_coeff = put(arena, "coeff", coeff_cells(k, n_cols))
    quot, rem = ctx.divide_columns(d_coeff, k, z, out=arena.out("quot", d_coeff.numel(), tuple(d_coeff.shape)), _rem=arena.out("rem", n_cols * 32, (n_cols, 32)),
                                   _workspace=workspace(pkg, arena, k, n_cols, 1))
    p_y = ctx.evaluate_columns(d_coeff, k, [y], out=arena.out("p_y", n_cols * 32, (n_cols, 1, 32)), _workspace=workspace(pkg, arena, k, n_cols, 1))
    q_y = ctx.evaluate_columns(quot, k, [y], out=arena.out("q_y", n_cols * 32, (n_cols, 1, 32)), _workspace=workspace(pkg, arena, k, n_cols, 1))
    arena.check()
    p_y, p_z, q_y = (nm.from_cells(t.cpu().numpy()) for t in (p_y, rem, q_y))
    assert [(a - b) % nm.R for a, b in zip(p_y, p_z)] == [q * (y - z) % nm.R for q in q_y]
    assert p_z == [om.evaluate(c, z) for c in columns(k, n_cols)] and len(set(q_y)) == n_cols


@pytest.mark.parametrize("mode", oc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(pkg, ctx, mode):
    k, n_cols, _ = oc.SHAPES[1]
    z = oc.points(k, 0x7074 + k)[-1]
    cols = [list(c) for c in columns(k, n_cols)]
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[mode % 2])
        d_coeff = put(arena, "coeff", coeff_cells(k, n_cols))
        quot, rem = ctx.divide_columns(d_coeff, k, z, out=arena.out("quot", d_coeff.numel(), tuple(d_coeff.shape)), _rem=arena.out("rem", n_cols * 32, (n_cols, 32)),
                                       _workspace=workspace(pkg, arena, k, n_cols, 1))
        folded = ctx.fold_columns(d_coeff, k, z, out=arena.out("folded", 32 << k, (1 << k, 32)))
        arena.check()
    finally:
        ctx.set_option("fr_store_mode", before)
    G.assert_bytes("divide, mode %d" % mode, quot.cpu().numpy(), divided(k, n_cols, z)[0])
    G.assert_bytes("the remainder, mode %d" % mode, rem.cpu().numpy(), divided(k, n_cols, z)[1])
    G.assert_bytes("fold, mode %d" % mode, folded.cpu().numpy(), nm.to_cells(om.fold(cols, z)))


def test_an_input_that_is_not_canonical_leaves_the_guard_bands_whole(pkg, ctx):
    k, n_cols, n_points = oc.SHAPES[1]
    ones = np.full((n_cols, 1 << k, 32), 0xFF, np.uint8)
    arena = G.DeviceArena()
    d_in = put(arena, "coeff", ones)
    d_points = put(arena, "points", np.full((n_points, 32), 0xFF, np.uint8))
    outs = [ctx.evaluate_columns(d_in, k, d_points, out=arena.out("evals", n_cols * n_points * 32, (n_cols, n_points, 32)),
                                 _workspace=workspace(pkg, arena, k, n_cols, n_points)),
            ctx.fold_columns(d_in, k, d_points[0], out=arena.out("folded", 32 << k, (1 << k, 32)))]
    outs += ctx.divide_columns(d_in, k, d_points[0], out=arena.out("quot", ones.size, ones.shape), _rem=arena.out("rem", n_cols * 32, (n_cols, 32)),
                               _workspace=workspace(pkg, arena, k, n_cols, 1))
    arena.check()
    G.assert_bytes("the input is left alone", d_in.cpu().numpy(), ones)
    for o in outs:  # every cell was written: no run of eight canary bytes is left (a cell of canaries is not canonical and not likely)
        assert not (o.cpu().numpy().reshape(-1, 8) == arena.canary).all(axis=1).any()


def test_every_refusal_leaves_the_poison_whole(pkg, ctx):
    import torch
    lib, api = pkg.api.load_open_library(), pkg.api
    k, n_cols, n_points = oc.SHAPES[1]
    arena = G.DeviceArena()
    d_in = put(arena, "coeff", coeff_cells(k, n_cols))
    d_points = put(arena, "points", nm.to_cells(oc.points(k, 1)[:n_points]))
    out = arena.out("out", n_cols * (32 << k))      # the quotient, the fold, the evaluations
    small = arena.out("small", n_cols * n_points * 32)  # the remainders
    ws = arena.out("ws", int(lib.aesw_open_workspace_bytes(k, n_cols, n_points)))
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    c, p, o, r, w = d_in.data_ptr(), d_points.data_ptr(), out.data_ptr(), small.data_ptr(), ws.data_ptr()
    call = lambda f, *a: getattr(lib, "aesw_open_%s_device" % f)(ctx._h, *a, s)  # noqa: E731
    refusals = [
        # evaluate: k, n_cols, n_points, d_coeff, d_points, d_evals, d_workspace
        ("evaluate", (9, n_cols, n_points, c, p, r, w), "k"), ("evaluate", (29, n_cols, n_points, c, p, r, w), "k"),
        ("evaluate", (k, 0, n_points, c, p, r, w), "n_cols"), ("evaluate", (k, 65536, n_points, c, p, r, w), "n_cols"),
        ("evaluate", (k, n_cols, 0, c, p, r, w), "n_points"), ("evaluate", (k, n_cols, 17, c, p, r, w), "n_points"),
        ("evaluate", (k, n_cols, n_points, None, p, r, w), "d_coeff"), ("evaluate", (k, n_cols, n_points, c, None, r, w), "d_points"),
        ("evaluate", (k, n_cols, n_points, c, p, None, w), "d_evals"), ("evaluate", (k, n_cols, n_points, c, p, r, None), "d_workspace"),
        ("evaluate", (k, n_cols, n_points, c + 8, p, r, w), "d_coeff"), ("evaluate", (k, n_cols, n_points, c, p + 4, r, w), "d_points"),
        ("evaluate", (k, n_cols, n_points, c, p, r + 8, w), "d_evals"), ("evaluate", (k, n_cols, n_points, c, p, r, w + 8), "d_workspace"),
        ("evaluate", (k, n_cols, n_points, o, p, o + 32, w), "overlap"),      # the evaluations lie in the columns
        ("evaluate", (k, n_cols, n_points, c, p, w + 64, w), "d_workspace"),  # the workspace overlaps an output
        ("evaluate", (k, n_cols, n_points, o, p, r, o + 64), "d_workspace"),  # ... and an input
        # fold: k, n_cols, d_coeff, d_v, d_acc_in, d_folded
        ("fold", (9, n_cols, c, p, None, o), "k"), ("fold", (29, n_cols, c, p, None, o), "k"),
        ("fold", (k, 0, c, p, None, o), "n_cols"), ("fold", (k, 65536, c, p, None, o), "n_cols"),
        ("fold", (k, n_cols, None, p, None, o), "d_coeff"), ("fold", (k, n_cols, c, None, None, o), "d_v"), ("fold", (k, n_cols, c, p, None, None), "d_folded"),
        ("fold", (k, n_cols, c + 8, p, None, o), "d_coeff"), ("fold", (k, n_cols, c, p + 8, None, o), "d_v"), ("fold", (k, n_cols, c, p, c + 8, o), "d_acc_in"),
        ("fold", (k, n_cols, c, p, None, o + 4), "d_folded"),
        ("fold", (k, n_cols, c, p, o + 32, o), "d_acc_in"),                   # a partial overlap of the accumulator and the result
        ("fold", (k, 2, o + 32, p, None, o), "overlap"),                      # the result lies in the columns
        # divide: k, n_cols, d_coeff, d_point, d_quot, d_rem, d_workspace
        ("divide", (9, n_cols, c, p, o, r, w), "k"), ("divide", (29, n_cols, c, p, o, r, w), "k"),
        ("divide", (k, 0, c, p, o, r, w), "n_cols"), ("divide", (k, 65536, c, p, o, r, w), "n_cols"),
        ("divide", (k, n_cols, None, p, o, r, w), "d_coeff"), ("divide", (k, n_cols, c, None, o, r, w), "d_point"), ("divide", (k, n_cols, c, p, None, r, w), "d_quot"),
        ("divide", (k, n_cols, c, p, o, None, w), "d_rem"), ("divide", (k, n_cols, c, p, o, r, None), "d_workspace"),
        ("divide", (k, n_cols, c + 8, p, o, r, w), "d_coeff"), ("divide", (k, n_cols, c, p + 8, o, r, w), "d_point"), ("divide", (k, n_cols, c, p, o + 8, r, w), "d_quot"),
        ("divide", (k, n_cols, c, p, o, r + 4, w), "d_rem"), ("divide", (k, n_cols, c, p, o, r, w + 8), "d_workspace"),
        ("divide", (k, 2, o + 32, p, o, r, w), "overlap"),                    # a partial overlap of the columns and the quotient
        ("divide", (k, n_cols, c, p, o, o + 64, w), "d_rem"),                 # the remainders lie in the quotient
        ("divide", (k, n_cols, c, p, o, w + 32, w), "d_workspace"),           # the workspace overlaps an output
    ]
    for f, args, word in refusals:
        assert call(f, *args) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_open_%s_device" % f) in err() and word in err(), (f, args, err())
    assert lib.aesw_open_evaluate_device(None, k, n_cols, n_points, c, p, r, w, s) == api.ERR_INVALID_ARG
    assert lib.aesw_open_fold_device(None, k, n_cols, c, p, None, o, s) == api.ERR_INVALID_ARG
    assert lib.aesw_open_divide_device(None, k, n_cols, c, p, o, r, w, s) == api.ERR_INVALID_ARG
    torch.cuda.synchronize()
    arena.check()
    assert arena.poisoned_on_device(out) and arena.poisoned_on_device(small) and arena.poisoned_on_device(ws)
    # the Python face says the same before it calls
    with pytest.raises(pkg.AeswError):
        ctx.evaluate_columns(d_in, 9, [1])
    with pytest.raises(ValueError):
        ctx.evaluate_columns(d_in, k + 1, [1])
    with pytest.raises(pkg.AeswError):
        ctx.evaluate_columns(d_in, k, list(range(17)))
    with pytest.raises(ValueError):
        ctx.divide_columns(d_in, k, [1, 2])
    with pytest.raises(ValueError):
        ctx.fold_columns(d_in, k, 1, acc=d_in)
    assert arena.poisoned_on_device(out)
