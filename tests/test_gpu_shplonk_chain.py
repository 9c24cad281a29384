"""SHPLONK's multi-opening over real columns on the GPU: the advice column and the lookup Z of tests/test_gpu_open_chain.py, in
coefficient form at its K, opened at rotated_points(x, K, sc.CHAIN_ROTATIONS) in three sets -- the advice column at x alone, Z at x
and x omega, and both once more at all three points.  Context.open_shplonk's two points and the proof bytes are held against
tests/shplonk_model.py driven by transcript_model (y, v, u) and msm_model (the two commitments, by the basis of known
logarithms); the report is clean.  Then the whole stage is captured once into a graph on a side stream and replayed twice: nothing
ran during capture, and each replay writes the same points and proof bytes."""
import numpy as np
import pytest

import msm_cases as mc
import msm_model as mm
import ntt_model as nm
import shplonk_cases as sc
import shplonk_model as sm
import transcript_model as tm
from test_gpu_open_chain import K, X, chain  # noqa: F401  (the fixture: one advice column and one Z as coefficients)

pytestmark = pytest.mark.gpu
QUERIES = [("advice", 0), ("z", 0), ("z", 1), ("z2", 0), ("z2", 1), ("z2", -1), ("advice2", -1), ("advice2", 0), ("advice2", 1)]


@pytest.fixture(scope="module")
def stage(pkg, ctx, chain):  # noqa: F811
    import torch
    plan = pkg.api.multiopen_plan(QUERIES)
    assert plan.rotations == list(sc.CHAIN_ROTATIONS) and plan.sets == [((0,), ["advice"]), ((0, 1), ["z"]), ((0, 1, 2), ["z2", "advice2"])]
    coeff, values = chain["coeff"], dict(advice=chain["values"][0], z=chain["values"][1], z2=chain["values"][1], advice2=chain["values"][0])
    points = pkg.api.rotated_points(X, K, plan.rotations)
    pts = nm.from_cells(points)
    evals = [[[nm.evaluate(values[c], pts[q]) for q in idx] for c in cols] for idx, cols in plan.sets]
    columns = [coeff[0:1], coeff[1:2], torch.stack([coeff[1], coeff[0]]).contiguous()]
    dev = coeff.device
    return dict(plan=plan, pts=pts, evals=evals, columns=columns, values=[[values[c] for c in cols] for _idx, cols in plan.sets],
                d_points=torch.from_numpy(points).to(dev), d_evals=torch.from_numpy(nm.to_cells(sc.flat_evals(evals))).to(dev),
                d_x=torch.from_numpy(pkg.api.fr_cell(X)).to(dev).view(1, 32), basis=torch.from_numpy(mc.basis_cells(K)).to(dev))


@pytest.fixture(scope="module")
def expected(stage):
    """(the model's opening, its two commitments, its transcript)"""
    s = stage
    t = tm.Transcript().common_scalars([X])
    y, v = t.squeeze(), t.squeeze()
    seen = {}

    def u_of(h):
        seen["h"] = mm.known_commit(h)
        t.write_points([seen["h"]])
        return t.squeeze()
    o = sm.opening(s["plan"], s["values"], s["evals"], s["pts"], y, v, u_of)
    seen["w"] = mm.known_commit(o["w"])
    t.write_points([seen["w"]])
    return o, [seen["h"], seen["w"]], t


def test_open_shplonk_gives_the_models_points_and_proof_bytes(pkg, ctx, stage, expected):
    s = stage
    o, commitments, model = expected
    t = ctx.transcript(64)
    t.common_scalars(s["d_x"])
    out, report = ctx.open_shplonk(s["plan"], s["columns"], s["d_evals"], s["d_points"], t, s["basis"])
    assert t.proof() == model.proof and len(model.proof) == 64
    assert pkg.api.g1_from_cells(out.cpu().numpy()) == commitments and commitments[0] != commitments[1] and None not in commitments
    rep = pkg.api.shplonk_report_dict(report)
    assert rep == dict(bad_sets=0, first_bad_set=None, zero_differences=0, z0_zero=0, last_remainder=[0, 0, 0, 0])
    assert o["report"]["bad_sets"] == 0 and o["report"]["last_remainder"] == 0 and any(o["w"]) and o["w"][-1] == 0
    assert t.status() == model.status(64)


def test_the_captured_stage_writes_the_same_bytes_through_two_replays(pkg, ctx, stage, expected):
    import torch
    s = stage
    _o, commitments, model = expected
    poison = 0xA5
    dev = s["basis"].device
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device=dev)  # noqa: E731
    state, proof, out, report = full(tm.STATE_BYTES), full(64), full(2, 64), full(64).view(torch.int64)
    t = ctx.transcript(64, _state=state, _proof=proof)
    torch.cuda.synchronize()
    state.fill_(poison)  # the constructor's init is not the stage's
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t.reset()
        t.common_scalars(s["d_x"])
        ctx.open_shplonk(s["plan"], s["columns"], s["d_evals"], s["d_points"], t, s["basis"], out=out, _report=report)
    torch.cuda.synchronize()
    assert all(bool((x.view(torch.uint8) == poison).all()) for x in (state, proof, out, report)), "the captured calls ran during capture"
    for _replay in range(2):
        for x in (proof, out):
            x.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert t.proof() == model.proof and pkg.api.g1_from_cells(out.cpu().numpy()) == commitments
        assert pkg.api.shplonk_report_dict(report)["bad_sets"] == 0 and np.array_equal(report.view(torch.uint8)[32:].cpu().numpy(), np.zeros(32, np.uint8))
