"""aesw_grand_invert_table_device / Context.invert_table on the GPU: all 2 x 3 x 66 561 cells of the inverse table against
tests/grand_model.py (pow(x, r - 2, r), 0 for 0) -- beta and gamma from two seeds (gc.CHALLENGE_SEEDS) next to 0, 1 and r - 1,
beta = -T_1[gc.ZERO_TERM_ROW] where the zero term must be counted and that cell must be zero, beta and, separately, gamma not
canonical (gc.NONCANONICAL).  The output sits in poisoned guard bands (tests/guarded.py); a refusal leaves it poisoned."""
import numpy as np
import pytest

import grand_cases as gc
import grand_model as gm
import guarded as G
import theta_model as tm

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
THETA = gc.seeded(gc.THETA_SEED)
S0, S1 = (gc.seeded(s) for s in gc.CHALLENGE_SEEDS)

_world = {}


def world(ctx, oracle):
    import torch
    if not _world:
        table = tm.compressed_tables(oracle.lookup_table(), THETA)
        d_table, rep = ctx.compress_table(THETA)
        assert not rep["noncanonical"] and np.array_equal(d_table.cpu().numpy(), table)
        _world.update(table=table, d_table=torch.from_numpy(table).cuda())
    return _world


def cell(value):
    import torch
    return torch.from_numpy(np.frombuffer(int(value).to_bytes(32, "little"), np.uint8).copy()).cuda()


def invert(pkg, ctx, arena, d_table, beta_cell, gamma_cell, expect=OK, over=None):
    import torch
    out = arena.out("inv", 2 * 3 * gm.BINS * 32, (2, 3, gm.BINS, 32))
    rep = arena.out("report", 24)
    args = dict(h=ctx._h, table=d_table.data_ptr(), beta=beta_cell.data_ptr(), gamma=gamma_cell.data_ptr(), out=out.data_ptr(), rep=rep.data_ptr())
    args.update(over or {})
    rc = pkg.api.load_grand_library().aesw_grand_invert_table_device(args["h"], args["table"], args["beta"], args["gamma"], args["out"], args["rep"], ctx._stream())
    assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
    torch.cuda.synchronize()
    return out, rep


def words(rep):
    import torch
    return rep.view(torch.int64)


def minus_t1(table):
    return (gm.R - gm.values(table[1][gc.ZERO_TERM_ROW])[0]) % gm.R


@pytest.mark.parametrize("case", ("seeds", "zero_one", "minus_one", "zero_term"))
def test_every_cell_of_the_inverse_table_is_the_models(pkg, ctx, oracle, case):
    w = world(ctx, oracle)
    beta, gamma = {"seeds": (S0, S1), "zero_one": (0, 1), "minus_one": (gm.R - 1, S0), "zero_term": (minus_t1(w["table"]), S1)}[case]
    assert gc.CHALLENGE_SEEDS and 0 <= gc.ZERO_TERM_ROW < gm.BINS
    exp, zeros = gm.inverse_tables(w["table"], beta, gamma)
    arena = G.DeviceArena(G.CANARIES[len(case) % 2])
    out, rep = invert(pkg, ctx, arena, w["d_table"], cell(beta * gm.M % gm.R), cell(gamma * gm.M % gm.R))
    got = out.cpu().numpy()
    bad = np.argwhere((got != exp).any(axis=3))
    assert not bad.size, "%s: %d cells differ, first (plane, table, row) %r" % (case, len(bad), bad[0].tolist())
    assert pkg.api.grand_invert_report_dict(words(rep)) == {"cells": 2 * 3 * gm.BINS, "noncanonical": False, "zero_terms": zeros}
    if case == "zero_one":
        assert zeros >= 3 and not got[0, :, gm.ZERO_ROW].any()  # beta = 0 meets the all-zero row of every table
    if case == "zero_term":
        assert zeros >= 1 and not got[0, 1, gc.ZERO_TERM_ROW].any() and got[1, 1, gc.ZERO_TERM_ROW].any()
    if case == "seeds":
        assert zeros == 0 and got.reshape(-1, 32).any(axis=1).all()
    arena.check_on_device()


@pytest.mark.parametrize("which", ("beta", "gamma"))
@pytest.mark.parametrize("value", gc.NONCANONICAL)
def test_a_challenge_that_is_not_canonical_zeroes_the_table_and_says_so(pkg, ctx, oracle, which, value):
    w = world(ctx, oracle)
    arena = G.DeviceArena()
    cells = {"beta": cell(S0 * gm.M % gm.R), "gamma": cell(S1 * gm.M % gm.R)}
    cells[which] = cell(value)
    out, rep = invert(pkg, ctx, arena, w["d_table"], cells["beta"], cells["gamma"])
    assert not out.any()
    assert pkg.api.grand_invert_report_dict(words(rep)) == {"cells": 2 * 3 * gm.BINS, "noncanonical": True, "zero_terms": 0}
    arena.check_on_device()


def test_the_python_face_and_the_refusals(pkg, ctx, oracle):
    import torch
    w = world(ctx, oracle)
    exp, zeros = gm.inverse_tables(w["table"], S0, S1)  # the model's memo: computed above
    inv, rep = ctx.invert_table(w["d_table"], S0, S1)
    assert np.array_equal(inv.cpu().numpy(), exp) and rep == {"cells": 2 * 3 * gm.BINS, "noncanonical": False, "zero_terms": zeros}
    inv2, rep2 = ctx.invert_table(w["d_table"], cell(S0 * gm.M % gm.R), S1 + gm.R, sync=False)  # a tensor as it lies; an int is reduced
    assert torch.equal(inv2, inv) and pkg.api.grand_invert_report_dict(rep2) == rep
    arena = G.DeviceArena()
    b, g = cell(S0), cell(S1)
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    outs = []
    for over, word in ((dict(table=None), "d_table_fr"), (dict(table=w["d_table"].data_ptr() + 8), "d_table_fr"), (dict(beta=None), "d_beta"),
                       (dict(gamma=g.data_ptr() + 4), "d_gamma"), (dict(out=None), "d_inv_fr"), (dict(rep=None), "d_report")):
        outs.extend(invert(pkg, ctx, arena, w["d_table"], b, g, expect=INVALID, over=over))
        assert "aesw_grand_invert_table_device" in err() and word in err(), (over, err())
    group = pkg.Group([0])
    try:
        outs.extend(invert(pkg, ctx, arena, w["d_table"], b, g, expect=INVALID, over=dict(h=group._h)))
        assert "aesw_grand_invert_table_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.invert_table(w["d_table"], 1, 2)
    finally:
        group.close()
    arena.check_on_device()
    assert all(arena.poisoned_on_device(t) for t in outs)
    with pytest.raises(ValueError):
        ctx.invert_table(w["d_table"][:2], 1, 2)
    with pytest.raises(ValueError):
        ctx.invert_table(w["d_table"], torch.zeros(31, dtype=torch.uint8, device="cuda"), 2)
