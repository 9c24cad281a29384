"""libaesw_shplonk.so where the sweep of tests/test_gpu_shplonk_columns.py never reaches: the second turn of the carry kernel.

sc.REACH_K = 19 is the smallest k whose column has more chunks (512) than the carry kernel scans a turn (256).  One set of one
column at t = 2 seeded points, on poisoned, guard-banded buffers: N_0 by combine_columns, every cell of v^0 Q_0 by set_quotient
and both remainders against ONE run of the model (two divisions of 2^19 cells in Python)."""
import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import open_model as om
import shplonk_cases as sc
import shplonk_model as sm

pytestmark = pytest.mark.gpu


def test_the_second_turn_of_the_carry_is_the_models(pkg, ctx):
    import torch
    k = sc.REACH_K
    n = 1 << k
    column = nm.seeded_values(n, 0x7372)
    pts = nm.seeded_values(2, 0x737a)
    y, v = nm.seeded_values(2, 0x7379)
    evals = [[[om.evaluate(column, z) for z in pts]]]
    plan = pkg.api.multiopen_plan([("c", 0), ("c", 1)])
    assert plan.sets == [((0, 1), ["c"])]
    prep = sm.prepare(plan, pts, evals, y, v)
    numer = sm.combine([column], prep["y_pow"], prep["sets"][0]["neg_r"])
    q, rems = sm.partial_quotient(numer, pts)
    assert rems == [0, 0] and q[-1] == q[-2] == 0 and q[-3] == column[-1]  # the degree drops by two
    lib = pkg.api.load_shplonk_library()
    arena = G.DeviceArena()
    cells = nm.to_cells(column).reshape(1, n, 32)
    d_column = arena.out("column", cells.size, cells.shape)
    d_column.copy_(torch.from_numpy(cells).to(d_column.device))
    scalars, report = ctx.shplonk_prepare(plan, pts, sc.flat_evals(evals), y, v, _scalars=arena.out("scalars", int(lib.aesw_shplonk_scalars_bytes(1, 1))),
                                          _report=arena.out("report", 64).view(torch.int64))
    d_numer = ctx.combine_columns(d_column, k, ctx.shplonk_table(scalars, "y_pow"), low=ctx.shplonk_table(scalars, "neg_r", 0, 2), out=arena.out("numer", 32 * n, (n, 32)))
    out, rem = ctx.set_quotient(d_numer, k, 0, pts, scalars, report, out=arena.out("out", 32 * n, (n, 32)), _rem=arena.out("rem", 256, (8, 32)),
                                _workspace=arena.out("ws", int(lib.aesw_shplonk_workspace_bytes(k))))
    arena.check()
    G.assert_bytes("N_0 at k = %d" % k, d_numer.cpu().numpy(), nm.to_cells(numer))
    G.assert_bytes("the quotient at k = %d" % k, out.cpu().numpy(), nm.to_cells(q))
    G.assert_bytes("the remainders", rem[:2].cpu().numpy(), nm.to_cells(rems))
    G.assert_bytes("the column is left alone", d_column.cpu().numpy(), cells)
    rep = pkg.api.shplonk_report_dict(report)
    assert (rep["bad_sets"], rep["first_bad_set"], rep["zero_differences"]) == (0, None, 0) and np.any(out[n - 3].cpu().numpy())
