"""libaesw_shplonk.so on the GPU at the extents its kernels are written for, against tests/shplonk_model.py, every written cell, on
poisoned, guard-banded buffers -- where the sweep of tests/test_gpu_shplonk_columns.py (4 sets over 8 points, at most 5 columns) does
not reach.

sc.FULL_SETS at k = 10: 16 sets over 16 super-set points, t = 1 ... 8, set 15 over the points 8 ... 15 alone, one set of 257 columns
(y^j past one stride of the prepare kernel's loop, exponents up to 256, evaluation offsets past 256): thread 16 of the finish
kernel, mask bits 8 ... 15, the strides of the [16][8] tables and the plan's words for the sets 4 ... 15, set_quotient above set 3.
u on a super-set point outside set 0 (z_0 = 0: the report says so, fr_inv(0) = 0 and L' is zero) and inside it (z_T = 0 alone).
y = 0, v = 0 and y = v = 1, each at u = 0 and at a seeded u, on sc.SETS.  A combine over 257 columns, in one call and in two.
The stage is run and held by run_stage and check_stage of tests/test_gpu_shplonk_columns.py."""
import functools

import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import shplonk_cases as sc
import shplonk_model as sm
from test_gpu_shplonk_columns import check_stage, put, run_stage

pytestmark = pytest.mark.gpu
K = sc.FULL_K


def stages():
    return {"full": sc.full_stage(), **sc.u_on_a_point(), **sc.degenerate_stages(K)}


@functools.lru_cache(maxsize=None)
def model(name):
    p, pts, columns, evals, y, v, u = stages()[name]
    return sm.opening(p, columns, evals, pts, y, v, lambda _h: u)


def table(ctx, scalars, name, cells, of_set=0):
    return nm.from_cells(ctx.shplonk_table(scalars, name, of_set, cells).cpu().numpy())


def test_the_full_plan_call_by_call_is_the_model(pkg, ctx):
    p, pts, _columns, _evals, _y, _v, _u = sc.full_stage()
    o = model("full")
    assert o["report"] == dict(bad_sets=0, first_bad_set=None, zero_differences=0, z0_zero=0, last_remainder=0)
    assert len(p.sets) == len(pts) == 16 and max(p.set_cols) == sc.WIDE_COLS
    got = run_stage(pkg, ctx, K, G.CANARIES[0], stage=sc.full_stage())
    # every table of the scalars block after prepare and after finish (v_pow 16 cells, the four [16][8] tables in full, z 16, l_coef
    # 17, y_pow 257), every N_i, every remainder with the rows from t_i on still poison, h, L' and a clean report
    check_stage(pkg, ctx, o, got, K)
    # the plan's words for every set: the mask, the first evaluation, the indices
    words = [int(w) for w in got["scalars"][:1024].cpu().numpy().view(np.uint32)]
    first, evals_at = 0, []
    for t, m in zip(p.set_points, p.set_cols):
        evals_at.append(first)
        first += t * m
    assert words[48:64] == [sum(1 << q for q in idx) for idx, _cols in p.sets] and words[64:80] == evals_at and max(evals_at) > 256
    assert [words[128 + 8 * i:136 + 8 * i] for i in range(16)] == [list(idx) + [0] * (8 - len(idx)) for idx, _cols in p.sets]
    assert table(ctx, got["scalars"], "l_coef", 1, 16) == [o["fin"]["l_coef"][16]] != [0] and table(ctx, got["scalars"], "z", 1, 15) == [o["fin"]["z"][15]]
    assert table(ctx, got["scalars"], "y_pow", sc.WIDE_COLS)[256] == pow(sc.full_stage()[4], 256, nm.R)
    for name in ("ebar", "w", "vw", "neg_r"):
        assert table(ctx, got["scalars"], name, 8, 15) == o["prep"]["sets"][15][name], name


def test_u_on_a_point_outside_set_0_is_reported_and_zeroes_the_line(pkg, ctx):
    name = "u_outside_set_0"
    p, pts, *_rest, u = sc.u_on_a_point()[name]
    o = model(name)
    assert pts.index(u) not in p.sets[0][0] and o["fin"]["z"][0] == 0 and o["report"]["z0_zero"] == 1
    assert o["fin"]["z0_inv"] == 0 and o["fin"]["l_coef"] == [0] * 17 and o["fin"]["l_low"] == [0] * 8 and not any(o["line"])  # the model: zero throughout
    got = run_stage(pkg, ctx, K, G.CANARIES[1], stage=sc.full_stage(), u=u)
    check_stage(pkg, ctx, o, got, K)
    assert pkg.api.shplonk_report_dict(got["report"])["z0_zero"] == 1
    assert table(ctx, got["scalars"], "z0_inv", 1) == [0] and table(ctx, got["scalars"], "l_coef", 17) == [0] * 17 and table(ctx, got["scalars"], "l_low", 8) == [0] * 8
    assert table(ctx, got["scalars"], "z", 16) == o["fin"]["z"] and any(o["fin"]["z"][1:])
    assert not got["line"].cpu().numpy().any()


def test_u_on_a_point_inside_set_0_zeroes_z_t_alone(pkg, ctx):
    name = "u_inside_set_0"
    p, pts, *_rest, u = sc.u_on_a_point()[name]
    o = model(name)
    assert pts.index(u) in p.sets[0][0] and o["fin"]["z_t"] == 0 and o["fin"]["z"][0] != 0 and o["report"]["z0_zero"] == 0 and any(o["line"])
    got = run_stage(pkg, ctx, K, G.CANARIES[0], stage=sc.full_stage(), u=u)
    check_stage(pkg, ctx, o, got, K)
    assert pkg.api.shplonk_report_dict(got["report"])["z0_zero"] == 0
    assert table(ctx, got["scalars"], "z_t", 1) == [0] and table(ctx, got["scalars"], "l_coef", 1, 16) == [0] and table(ctx, got["scalars"], "z0_inv", 1) == [o["fin"]["z0_inv"]] != [0]


@pytest.mark.parametrize("name", sorted(sc.degenerate_stages(K)))
def test_challenges_of_0_and_1_give_the_models_cells(pkg, ctx, name):
    stage = sc.degenerate_stages(K)[name]
    p, _pts, columns, _evals, y, v, u = stage
    o = model(name)
    if y == 0:  # 0^0 is 1: N_i is the first column of set i plus the low cells
        assert o["prep"]["y_pow"] == [1, 0, 0, 0, 0]
        assert all(o["numer"][i] == sm.combine(columns[i][:1], [1], s["neg_r"]) for i, s in enumerate(o["prep"]["sets"]))
    if v == 0:  # h is the scaled quotient of set 0 alone
        assert o["prep"]["v_pow"] == [1, 0, 0, 0] and o["h"] == sm.partial_quotient(o["numer"][0], o["prep"]["sets"][0]["pts"])[0] and any(o["h"])
    assert o["report"]["z0_zero"] == int(u == 0) and o["report"]["bad_sets"] == 0
    canary = G.CANARIES[sorted(sc.degenerate_stages(K)).index(name) % 2]
    check_stage(pkg, ctx, o, run_stage(pkg, ctx, K, canary, stage=stage), K)


def test_a_combine_over_257_columns_in_one_call_and_in_two(pkg, ctx):
    columns = sc.full_stage()[2][sc.WIDE_SET]
    coefs = nm.seeded_values(sc.WIDE_COLS, 0x636f6566)
    assert len(columns) == sc.WIDE_COLS == 257
    n = 1 << K
    arena = G.DeviceArena(G.CANARIES[1])
    d_cols = put(arena, "cols", np.stack([nm.to_cells(c) for c in columns]))
    new = lambda name: arena.out(name, 32 * n, (n, 32))  # noqa: E731
    whole = ctx.combine_columns(d_cols, K, coefs, out=new("whole"))
    first = ctx.combine_columns(d_cols[:256], K, coefs[:256], out=new("first"))
    second = ctx.combine_columns(d_cols[256:], K, coefs[256:], acc=first, out=first)
    arena.check()
    assert second.data_ptr() == first.data_ptr()
    G.assert_bytes("257 columns in one call", whole.cpu().numpy(), nm.to_cells(sm.combine(columns, coefs)))
    G.assert_bytes("256 columns and one more", second.cpu().numpy(), whole.cpu().numpy())
    G.assert_bytes("the columns are left alone", d_cols.cpu().numpy(), np.stack([nm.to_cells(c) for c in columns]))
