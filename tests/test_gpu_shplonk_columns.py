"""libaesw_shplonk.so on the GPU against tests/shplonk_model.py, every written cell, on poisoned, guard-banded buffers.

sc.KS: k = 10 (one chunk) and k = 11 (the carry is crossed); sc.SETS: t = 1, 2, 3 and 8, m = 5 and 1, over the points 0, 1, omega_k,
r - 1 and four seeded values.  Every cell of both scalar phases, of combine (N_i and L') and of set_quotient; acc absent, separate
and in place; d_out == d_numer; the three fr_store_modes; a set with one wrong evaluation (report and remainder exact); two equal
points in a set (counted, stores in bounds); every refusal."""
import functools

import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import open_model as om
import shplonk_cases as sc
import shplonk_model as sm

pytestmark = pytest.mark.gpu
R = nm.R


def put(arena, name, cells):
    """a guarded, 16-byte aligned device copy of uint8 cells"""
    import torch
    t = arena.out(name, cells.size, cells.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(cells)).to(t.device))
    return t


@functools.lru_cache(maxsize=None)
def model(k, wrong=None):
    p, pts, columns, evals, y, v, u = sc.stage(k, wrong=wrong)
    return sm.opening(p, columns, evals, pts, y, v, lambda _h: u)


def pad(rows):
    return [x for row in rows for x in list(row) + [0] * (8 - len(row))] + [0] * (8 * (16 - len(rows)))


def check_prepared(ctx, p, o, scalars):
    prep, S = o["prep"], len(p.sets)
    words = scalars[:1024].cpu().numpy().view(np.uint32)
    assert list(words[:3]) == [len(p.rotations), S, max(p.set_cols)] and list(words[16:16 + S]) == p.set_points and list(words[32:32 + S]) == p.set_cols
    table = lambda name, cells, of_set=0: nm.from_cells(ctx.shplonk_table(scalars, name, of_set, cells).cpu().numpy())  # noqa: E731
    assert table("y_pow", max(p.set_cols)) == prep["y_pow"] and table("v_pow", 16) == prep["v_pow"] + [0] * (16 - S)
    for name in ("ebar", "w", "vw", "neg_r"):
        assert table(name, 128) == pad([s[name] for s in prep["sets"]]), name


def check_finished(ctx, p, o, scalars):
    fin, S = o["fin"], len(p.sets)
    table = lambda name, cells, of_set=0: nm.from_cells(ctx.shplonk_table(scalars, name, of_set, cells).cpu().numpy())  # noqa: E731
    assert table("z", 16) == fin["z"] + [0] * (16 - S) and table("z_t", 1) == [fin["z_t"]] and table("z0_inv", 1) == [fin["z0_inv"]]
    assert table("l_coef", 17) == fin["l_coef"] + [0] * (16 - S) and table("l_const", 1) == [fin["l_const"]] and table("l_low", 8) == fin["l_low"]
    assert table("l_coef", 1, S) == [fin["l_coef"][S]]


def run_stage(pkg, ctx, k, canary, wrong=None, moved=None, in_place_numer=False, stage=None, u=None):
    """the stage call by call on guarded buffers; returns what the calls wrote.  moved: (points, evals) to take instead of the stage's;
    stage: a tuple of sc.stage's shape to take instead of sc.stage(k, wrong=wrong); u: the last challenge instead of the stage's"""
    api = pkg.api
    lib = api.load_shplonk_library()
    p, pts, columns, evals, y, v, own_u = sc.stage(k, wrong=wrong) if stage is None else stage
    u = own_u if u is None else u
    pts, evals = moved if moved is not None else (pts, evals)
    plan = api.MultiopenPlan(p.rotations, p.sets)
    S, n = len(p.sets), 1 << k
    arena = G.DeviceArena(canary)
    d_points = put(arena, "points", nm.to_cells(pts))
    d_evals = put(arena, "evals", nm.to_cells(sc.flat_evals(evals)))
    d_y, d_v, d_u = (put(arena, name, nm.to_cells([x]).reshape(32)) for name, x in (("y", y), ("v", v), ("u", u)))
    need = int(lib.aesw_shplonk_scalars_bytes(S, max(p.set_cols)))
    scalars, report = ctx.shplonk_prepare(plan, d_points, d_evals, d_y, d_v, _scalars=arena.out("scalars", need), _report=arena.out("report", 64).view(ctx._torch().int64))
    arena.check()
    after_prepare = scalars.clone()
    ws = arena.out("ws", int(lib.aesw_shplonk_workspace_bytes(k)))
    numer, rems = [], []
    h = arena.out("h", 32 * n, (n, 32))
    for i in range(S):
        d_cols = put(arena, "cols%d" % i, np.stack([nm.to_cells(c) for c in columns[i]]))
        n_i = ctx.combine_columns(d_cols, k, ctx.shplonk_table(scalars, "y_pow", cells=p.set_cols[i]), low=ctx.shplonk_table(scalars, "neg_r", i, p.set_points[i]),
                                  out=arena.out("numer%d" % i, 32 * n, (n, 32)))
        rem = arena.out("rem%d" % i, 256, (8, 32))
        if in_place_numer and i == 0:  # the first set: no accumulator, and the quotient over its own numerator
            kept = n_i.clone()
            ctx.set_quotient(n_i, k, i, d_points, scalars, report, out=n_i, _rem=rem, _workspace=ws)
            h.copy_(n_i)
            n_i = kept
        else:
            ctx.set_quotient(n_i, k, i, d_points, scalars, report, acc=h if i else None, out=h, _rem=rem, _workspace=ws)  # h accumulates in place
        numer.append(n_i)
        rems.append(rem)
    ctx.shplonk_finish(d_points, d_u, scalars, report)
    work = put(arena, "work", np.concatenate([t.cpu().numpy() for t in numer] + [h.cpu().numpy()]).reshape(S + 1, n, 32))
    line = ctx.combine_columns(work, k, ctx.shplonk_table(scalars, "l_coef", cells=S + 1), low=ctx.shplonk_table(scalars, "l_low", cells=8), out=arena.out("line", 32 * n, (n, 32)))
    arena.check()
    return dict(plan=p, arena=arena, after_prepare=after_prepare, scalars=scalars, report=report, numer=numer, rems=rems, h=h, line=line, points=d_points, ws=ws, work=work)


def check_stage(pkg, ctx, o, got, k):
    p = got["plan"]
    check_prepared(ctx, p, o, got["after_prepare"])
    check_prepared(ctx, p, o, got["scalars"])  # the finish call leaves the first phase's tables alone
    check_finished(ctx, p, o, got["scalars"])
    for i, (n_i, rem) in enumerate(zip(got["numer"], got["rems"])):
        G.assert_bytes("N_%d at k = %d" % (i, k), n_i.cpu().numpy(), nm.to_cells(o["numer"][i]))
        t = p.set_points[i]
        G.assert_bytes("the remainders of set %d" % i, rem[:t].cpu().numpy(), nm.to_cells(o["rems"][i]))
        assert got["arena"].poisoned(rem[t:]) or t == 8  # the cells past t_i are left alone
    G.assert_bytes("h at k = %d" % k, got["h"].cpu().numpy(), nm.to_cells(o["h"]))
    G.assert_bytes("L' at k = %d" % k, got["line"].cpu().numpy(), nm.to_cells(o["line"]))
    rep = pkg.api.shplonk_report_dict(got["report"])
    want = o["report"]
    assert (rep["bad_sets"], rep["first_bad_set"], rep["zero_differences"], rep["z0_zero"]) == (want["bad_sets"], want["first_bad_set"], want["zero_differences"], want["z0_zero"])
    assert rep["last_remainder"] == [0, 0, 0, 0]  # the prepare call zeroed it; the last division is the caller's


@pytest.mark.parametrize("k", sc.KS)
def test_every_cell_of_the_stage_is_the_model(pkg, ctx, k):
    o = model(k)
    assert o["report"]["bad_sets"] == 0 and o["report"]["last_remainder"] == 0
    for canary, in_place in zip(G.CANARIES, (False, True)):
        check_stage(pkg, ctx, o, run_stage(pkg, ctx, k, canary, in_place_numer=in_place), k)


def test_the_accumulator_absent_separate_and_in_place(pkg, ctx):
    k = sc.KS[1]
    o = model(k)
    got = run_stage(pkg, ctx, k, G.CANARIES[0])
    arena, n = got["arena"], 1 << k
    p, pts, *_ = sc.stage(k)
    acc = nm.seeded_values(n, 0x6163)
    d_acc = put(arena, "acc", nm.to_cells(acc))
    new = lambda name: arena.out(name, 32 * n, (n, 32))  # noqa: E731
    rem = lambda: arena.out("rem", 256, (8, 32))  # noqa: E731
    i = 3  # t = 8
    q, _rems = sm.partial_quotient(o["numer"][i], [pts[x] for x in p.sets[i][0]])
    scaled = [o["prep"]["v_pow"][i] * c % R for c in q]
    bare, _ = ctx.set_quotient(got["numer"][i], k, i, got["points"], got["scalars"], got["report"], out=new("bare"), _rem=rem(), _workspace=got["ws"])
    separate, _ = ctx.set_quotient(got["numer"][i], k, i, got["points"], got["scalars"], got["report"], acc=d_acc, out=new("separate"), _rem=rem(), _workspace=got["ws"])
    same = put(arena, "same", nm.to_cells(acc))
    ctx.set_quotient(got["numer"][i], k, i, got["points"], got["scalars"], got["report"], acc=same, out=same, _rem=rem(), _workspace=got["ws"])
    # the combine: no accumulator, one of its own, one in place; two calls of 3 + 2 columns against one of 5
    columns = sc.stage(k)[2][0]
    d_cols = put(arena, "cols", np.stack([nm.to_cells(c) for c in columns]))
    coefs = nm.seeded_values(5, 0x636f)
    c_bare = ctx.combine_columns(d_cols, k, coefs, out=new("c_bare"))
    c_low = ctx.combine_columns(d_cols, k, coefs, low=[7, 8, 9], acc=d_acc, out=new("c_low"))
    first = ctx.combine_columns(d_cols[:3], k, coefs[:3], low=[7, 8, 9], acc=d_acc, out=new("first"))
    second = ctx.combine_columns(d_cols[3:], k, coefs[3:], acc=first, out=first)
    arena.check()
    assert second.data_ptr() == first.data_ptr()
    G.assert_bytes("quotient without acc", bare.cpu().numpy(), nm.to_cells(scaled))
    G.assert_bytes("quotient with acc", separate.cpu().numpy(), nm.to_cells([(a + c) % R for a, c in zip(acc, scaled)]))
    G.assert_bytes("quotient into acc", same.cpu().numpy(), separate.cpu().numpy())
    G.assert_bytes("the accumulator is left alone", d_acc.cpu().numpy(), nm.to_cells(acc))
    G.assert_bytes("the numerator is left alone", got["numer"][i].cpu().numpy(), nm.to_cells(o["numer"][i]))
    G.assert_bytes("combine without acc", c_bare.cpu().numpy(), nm.to_cells(sm.combine(columns, coefs)))
    G.assert_bytes("combine with acc and low cells", c_low.cpu().numpy(), nm.to_cells(sm.combine(columns, coefs, [7, 8, 9], acc)))
    G.assert_bytes("two combines are one", second.cpu().numpy(), c_low.cpu().numpy())
    G.assert_bytes("the columns are left alone", d_cols.cpu().numpy(), np.stack([nm.to_cells(c) for c in columns]))


@pytest.mark.parametrize("mode", sc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(pkg, ctx, mode):
    k = sc.KS[1]
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        got = run_stage(pkg, ctx, k, G.CANARIES[mode % 2])
    finally:
        ctx.set_option("fr_store_mode", before)
    check_stage(pkg, ctx, model(k), got, k)


def test_a_wrong_evaluation_is_reported_and_the_quotient_is_still_the_partial_sum(pkg, ctx):
    k, wrong = sc.KS[1], (2, 0, 1)
    o = model(k, wrong)
    assert o["report"]["bad_sets"] == 1 and o["report"]["first_bad_set"] == 2 and [bool(r) for r in o["rems"][2]] == [False, True, False]
    # R_2 lies below Z_2's degree, so the quotient does not see it: h stays, N_2, its remainder and L' move
    assert o["h"] == model(k)["h"] and o["numer"][2] != model(k)["numer"][2] and o["line"] != model(k)["line"]
    check_stage(pkg, ctx, o, run_stage(pkg, ctx, k, G.CANARIES[1], wrong=wrong), k)


def test_two_equal_points_in_a_set_are_counted_and_every_store_stays_in_bounds(pkg, ctx):
    k = sc.KS[0]
    p, pts, columns, _evals, y, v, u = sc.stage(k)
    pts = list(pts)
    pts[6] = pts[5]  # set 3 holds both
    evals = [[[om.evaluate(column, pts[q]) for q in idx] for column in columns[i]] for i, (idx, _cols) in enumerate(p.sets)]
    o = sm.opening(p, columns, evals, pts, y, v, lambda _h: u)
    assert o["report"]["zero_differences"] == 2 and o["prep"]["sets"][3]["w"][5] == o["prep"]["sets"][3]["w"][6] == 0
    check_stage(pkg, ctx, o, run_stage(pkg, ctx, k, G.CANARIES[0], moved=(pts, evals)), k)


def test_every_refusal_leaves_the_poison_whole(pkg, ctx):
    import ctypes as C
    import torch
    lib, api = pkg.api.load_shplonk_library(), pkg.api
    k = sc.KS[1]
    n = 1 << k
    p, pts, columns, evals, y, v, u = sc.stage(k)
    arena = G.DeviceArena()
    d_points = put(arena, "points", nm.to_cells(pts))
    d_evals = put(arena, "evals", nm.to_cells(sc.flat_evals(evals)))
    d_cells = put(arena, "cells", nm.to_cells([y, v, u]))
    d_cols = put(arena, "cols", np.stack([nm.to_cells(c) for c in columns[0]]))
    scalars = arena.out("scalars", int(lib.aesw_shplonk_scalars_bytes(4, 5)))
    report = arena.out("report", 64)
    out, rem = arena.out("out", 2 * 32 * n), arena.out("rem", 256)
    ws = arena.out("ws", int(lib.aesw_shplonk_workspace_bytes(k)))
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    words = lambda a: (C.c_uint32 * len(a))(*a)  # noqa: E731
    T, M, IDX = words(p.set_points), words(p.set_cols), words(p.point_index)
    P, E, Y, V, U, c, S_, r, o, m, w = (t.data_ptr() for t in (d_points, d_evals, d_cells[0], d_cells[1], d_cells[2], d_cols, scalars, report, out, rem, ws))
    call = lambda f, *a: getattr(lib, "aesw_shplonk_%s_device" % f)(ctx._h, *a, s)  # noqa: E731
    refusals = [
        # prepare: n_points, n_sets, set_points, set_cols, point_index, d_points, d_evals, d_y, d_v, d_scalars, d_report
        ("prepare", (0, 4, T, M, IDX, P, E, Y, V, S_, r), "n_points"), ("prepare", (17, 4, T, M, IDX, P, E, Y, V, S_, r), "n_points"),
        ("prepare", (8, 0, T, M, IDX, P, E, Y, V, S_, r), "n_sets"), ("prepare", (8, 17, T, M, IDX, P, E, Y, V, S_, r), "n_sets"),
        ("prepare", (8, 4, None, M, IDX, P, E, Y, V, S_, r), "set_points"), ("prepare", (8, 4, T, None, IDX, P, E, Y, V, S_, r), "set_cols"),
        ("prepare", (8, 4, T, M, None, P, E, Y, V, S_, r), "point_index"),
        ("prepare", (8, 4, words([0, 2, 3, 8]), M, IDX, P, E, Y, V, S_, r), "set_points"), ("prepare", (8, 4, words([9, 2, 3, 8]), M, IDX, P, E, Y, V, S_, r), "set_points"),
        ("prepare", (8, 4, T, words([5, 0, 1, 5]), IDX, P, E, Y, V, S_, r), "set_cols"), ("prepare", (8, 4, T, words([5, 65536, 1, 5]), IDX, P, E, Y, V, S_, r), "set_cols"),
        ("prepare", (4, 4, T, M, IDX, P, E, Y, V, S_, r), "below n_points"), ("prepare", (8, 2, words([1, 2]), M, words([4, 1, 1]), P, E, Y, V, S_, r), "increasing"),
        ("prepare", (8, 2, words([1, 2]), M, words([4, 3, 1]), P, E, Y, V, S_, r), "increasing"),
        ("prepare", (8, 4, T, M, IDX, None, E, Y, V, S_, r), "d_points"), ("prepare", (8, 4, T, M, IDX, P, None, Y, V, S_, r), "d_evals"),
        ("prepare", (8, 4, T, M, IDX, P, E, None, V, S_, r), "d_y"), ("prepare", (8, 4, T, M, IDX, P, E, Y, None, S_, r), "d_v"),
        ("prepare", (8, 4, T, M, IDX, P, E, Y, V, None, r), "d_scalars"), ("prepare", (8, 4, T, M, IDX, P, E, Y, V, S_, None), "d_report"),
        ("prepare", (8, 4, T, M, IDX, P + 8, E, Y, V, S_, r), "d_points"), ("prepare", (8, 4, T, M, IDX, P, E + 4, Y, V, S_, r), "d_evals"),
        ("prepare", (8, 4, T, M, IDX, P, E, Y + 8, V, S_, r), "d_y"), ("prepare", (8, 4, T, M, IDX, P, E, Y, V + 8, S_, r), "d_v"),
        ("prepare", (8, 4, T, M, IDX, P, E, Y, V, S_ + 8, r), "d_scalars"), ("prepare", (8, 4, T, M, IDX, P, E, Y, V, S_, r + 8), "d_report"),
        ("prepare", (8, 4, T, M, IDX, S_ + 64, E, Y, V, S_, r), "overlap"), ("prepare", (8, 4, T, M, IDX, P, E, Y, S_ + 32, S_, r), "overlap"),
        ("prepare", (8, 4, T, M, IDX, P, E, Y, V, S_, S_ + 2048), "d_report"),
        # finish: d_points, d_u, d_scalars, d_report
        ("finish", (None, U, S_, r), "d_points"), ("finish", (P, None, S_, r), "d_u"), ("finish", (P, U, None, r), "d_scalars"), ("finish", (P, U, S_, None), "d_report"),
        ("finish", (P + 8, U, S_, r), "d_points"), ("finish", (P, U + 4, S_, r), "d_u"), ("finish", (P, U, S_ + 8, r), "d_scalars"), ("finish", (P, U, S_, r + 8), "d_report"),
        ("finish", (P, S_ + 32, S_, r), "overlap"), ("finish", (P, U, S_, S_ + 1024), "d_report"),
        # combine: k, n_cols, d_coeff, d_coefs, d_low, n_low, d_acc_in, d_out
        ("combine", (9, 5, c, Y, None, 0, None, o), "k"), ("combine", (29, 5, c, Y, None, 0, None, o), "k"),
        ("combine", (k, 0, c, Y, None, 0, None, o), "n_cols"), ("combine", (k, 65536, c, Y, None, 0, None, o), "n_cols"),
        ("combine", (k, 5, c, Y, P, 9, None, o), "n_low"), ("combine", (k, 5, c, Y, None, 1, None, o), "d_low"), ("combine", (k, 5, c, Y, P, 0, None, o), "d_low"),
        ("combine", (k, 5, None, Y, None, 0, None, o), "d_coeff"), ("combine", (k, 5, c, None, None, 0, None, o), "d_coefs"), ("combine", (k, 5, c, Y, None, 0, None, None), "d_out"),
        ("combine", (k, 5, c + 8, Y, None, 0, None, o), "d_coeff"), ("combine", (k, 5, c, Y + 8, None, 0, None, o), "d_coefs"), ("combine", (k, 5, c, Y, P + 8, 1, None, o), "d_low"),
        ("combine", (k, 5, c, Y, None, 0, c + 8, o), "d_acc_in"), ("combine", (k, 5, c, Y, None, 0, None, o + 4), "d_out"),
        ("combine", (k, 5, c, Y, None, 0, o + 32, o), "d_acc_in"), ("combine", (k, 2, o + 32, Y, None, 0, None, o), "overlap"), ("combine", (k, 1, c, o + 64, None, 0, None, o), "overlap"),
        # quotient: k, set, d_numer, d_points, d_scalars, d_acc_in, d_out, d_rem, d_workspace, d_report
        ("quotient", (9, 0, c, P, S_, None, o, m, w, r), "k"), ("quotient", (29, 0, c, P, S_, None, o, m, w, r), "k"), ("quotient", (k, 16, c, P, S_, None, o, m, w, r), "set"),
        ("quotient", (k, 0, None, P, S_, None, o, m, w, r), "d_numer"), ("quotient", (k, 0, c, None, S_, None, o, m, w, r), "d_points"),
        ("quotient", (k, 0, c, P, None, None, o, m, w, r), "d_scalars"), ("quotient", (k, 0, c, P, S_, None, None, m, w, r), "d_out"),
        ("quotient", (k, 0, c, P, S_, None, o, None, w, r), "d_rem"), ("quotient", (k, 0, c, P, S_, None, o, m, None, r), "d_workspace"),
        ("quotient", (k, 0, c, P, S_, None, o, m, w, None), "d_report"),
        ("quotient", (k, 0, c + 8, P, S_, None, o, m, w, r), "d_numer"), ("quotient", (k, 0, c, P + 8, S_, None, o, m, w, r), "d_points"),
        ("quotient", (k, 0, c, P, S_ + 8, None, o, m, w, r), "d_scalars"), ("quotient", (k, 0, c, P, S_, c + 8, o, m, w, r), "d_acc_in"),
        ("quotient", (k, 0, c, P, S_, None, o + 8, m, w, r), "d_out"), ("quotient", (k, 0, c, P, S_, None, o, m + 8, w, r), "d_rem"),
        ("quotient", (k, 0, c, P, S_, None, o, m, w + 8, r), "d_workspace"), ("quotient", (k, 0, c, P, S_, None, o, m, w, r + 8), "d_report"),
        ("quotient", (k, 0, o + 32, P, S_, None, o, m, w, r), "d_numer"),       # a partial overlap of the numerator and the result
        ("quotient", (k, 0, c, P, S_, o + 32, o, m, w, r), "d_acc_in"),         # ... of the accumulator and the result
        ("quotient", (k, 0, c, P, S_, None, o, o + 64, w, r), "d_rem"),         # the remainders lie in the result
        ("quotient", (k, 0, c, P, S_, None, o, m, m + 32, r), "d_workspace"),   # the workspace overlaps the remainders
        ("quotient", (k, 0, c, P, S_, None, o, m, w, w + 64), "d_report"),      # the report lies in the workspace
    ]
    for f, args, word in refusals:
        assert call(f, *args) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_shplonk_%s_device" % f) in err() and word in err(), (f, args, err())
    assert lib.aesw_shplonk_prepare_device(None, 8, 4, T, M, IDX, P, E, Y, V, S_, r, s) == api.ERR_INVALID_ARG
    assert lib.aesw_shplonk_finish_device(None, P, U, S_, r, s) == api.ERR_INVALID_ARG
    assert lib.aesw_shplonk_combine_device(None, k, 5, c, Y, None, 0, None, o, s) == api.ERR_INVALID_ARG
    assert lib.aesw_shplonk_quotient_device(None, k, 0, c, P, S_, None, o, m, w, r, s) == api.ERR_INVALID_ARG
    torch.cuda.synchronize()
    arena.check()
    assert all(arena.poisoned_on_device(t) for t in (scalars, report, out, rem, ws))
    # the Python face says the same before it calls
    plan = api.MultiopenPlan(p.rotations, p.sets)
    with pytest.raises(ValueError):
        ctx.shplonk_prepare(plan, d_points[:7], d_evals, y, v)
    with pytest.raises(ValueError):
        ctx.shplonk_prepare(plan, d_points, d_evals[:-1], y, v)
    with pytest.raises(pkg.AeswError):
        ctx.shplonk_prepare(api.MultiopenPlan([], []), [], [], y, v)
    with pytest.raises(ValueError):
        ctx.combine_columns(d_cols, k, [1, 2, 3])
    with pytest.raises(pkg.AeswError):
        ctx.combine_columns(d_cols, 9, [1, 2, 3, 4, 5])
    with pytest.raises(pkg.AeswError):
        ctx.shplonk_table(scalars, "z_t", 1)
    assert arena.poisoned_on_device(out) and arena.poisoned_on_device(scalars)
