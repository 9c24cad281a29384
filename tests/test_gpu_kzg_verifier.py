"""The proof stage on the GPU under a verifier: what the device writes -- commitments, proof bytes, [h] and [W] -- held by
tests/kzg_verifier.py, which knows none of the prover's tables and shares no rule with tests/shplonk_model.py or open_model.py.

Everything at k = 10, the smallest the multi-scalar product takes, against the bases tau^i G and L_i(tau) G of a tau the test
knows, so that a commitment is f(tau) G and an opening is a group equation:

  * commit_columns(coeff, tau_basis) is evaluate_columns(coeff, [tau]) times G: libaesw_msm.so against libaesw_open.so, and both
    against Python's Horner sum; the zero column is the identity on both sides;
  * a column commits to one point in Lagrange and in coefficient form, through lagrange_to_coeff and through coeff_to_lagrange:
    seeded cells, a column that is 1 at one row (that basis point) and a constant column (c G), with slices = 0 and 3;
  * divide_columns' quotient, committed, opens the column's commitment at x to the device's remainder (x seeded, 0 and omega_10),
    and to nothing else;
  * a whole stage -- write_points of the commitments, x, evaluate_columns, write_scalars, open_shplonk -- is accepted from
    t.proof() and the plan alone: the verifier recomputes x, the points, y, v and u.  With one evaluation raised by 1 before it is
    written the device's report names the set and the verifier rejects the bytes;
  * sc.full_stage() -- 16 sets, 16 points, 257 columns in one set -- call by call as tests/test_gpu_shplonk_extents.py runs it:
    [h] and [W] committed on the device, the 274 columns' commitments formed by their exponents on the host.

Outputs lie in poisoned, guard-banded buffers (tests/guarded.py)."""
import numpy as np
import pytest

import guarded as G
import kzg_verifier as kv
import msm_cases as mc
import msm_model as mm
import ntt_model as nm
import shplonk_cases as sc
from test_gpu_msm_columns import commit, put
from test_gpu_shplonk_chain import QUERIES
from test_gpu_shplonk_columns import run_stage

pytestmark = pytest.mark.gpu
K, N, R, TAU = 10, 1 << 10, nm.R, kv.TAU
ROW, CONSTANT = 700, nm.seeded_values(1, 0x636f6e)[0]


@pytest.fixture(scope="module")
def bases(ctx):
    """the two bases on the device, built once by the verifier's fixed-base table"""
    import torch
    return {"tau": torch.from_numpy(mm.to_points(kv.tau_basis(K, TAU))).cuda(), "lagrange": torch.from_numpy(mm.to_points(kv.lagrange_basis(K, TAU))).cuda()}


def cells(columns):
    return np.stack([nm.to_cells(c) for c in columns])


def points_of(pkg, got):
    return pkg.api.g1_from_cells(got)


def test_a_commitment_is_an_evaluation_at_tau(pkg, ctx, bases):
    columns = [nm.seeded_values(N, 0x6b7a30 + j) for j in range(3)] + [[0] * N]
    arena = G.DeviceArena(G.CANARIES[0])
    committed = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, cells(columns), bases["tau"], 0))
    d_coeff = put(arena, "coeff", cells(columns))
    ws = arena.out("ws", int(pkg.api.load_open_library().aesw_open_workspace_bytes(K, 4, 1)))
    at_tau = ctx.evaluate_columns(d_coeff, K, [TAU], out=arena.out("evals", 4 * 32, (4, 1, 32)), _workspace=ws)
    arena.check()
    at_tau = nm.from_cells(at_tau.cpu().numpy())
    assert committed == [kv.fixed_mul(e) for e in at_tau]                       # the two libraries, with no model between them
    assert at_tau == [kv.evaluate(c, TAU) for c in columns] and at_tau[3] == 0  # and both against Python
    assert committed[3] is None and None not in committed[:3] and len(set(committed)) == 4


@pytest.mark.parametrize("slices", (0, 3))
def test_lagrange_and_coefficient_commitments_agree(pkg, ctx, bases, slices):
    unit, constant = [int(i == ROW) for i in range(N)], [CONSTANT] * N
    columns = [nm.seeded_values(N, 0x6b7a40), unit, constant, nm.seeded_values(N, 0x6b7a41)]
    arena = G.DeviceArena(G.CANARIES[slices % 2])
    tables = ctx.ntt_tables(K)
    d_cells = put(arena, "cells", cells(columns))
    new = lambda name: arena.out(name, 4 * N * 32, (4, N, 32))  # noqa: E731
    # as cells over the Lagrange basis, and as their coefficients over the powers of tau
    as_coeff = ctx.lagrange_to_coeff(d_cells, K, tables, out=new("coeff"))
    of_cells = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, d_cells.cpu().numpy(), bases["lagrange"], slices))
    of_coeff = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, as_coeff.cpu().numpy(), bases["tau"], slices))
    assert of_cells == of_coeff and None not in of_cells and len(set(of_cells)) == 4
    assert of_cells[1] == kv.lagrange_basis(K, TAU)[ROW] and of_cells[2] == kv.fixed_mul(CONSTANT)
    l_at = kv.lagrange_at(K, TAU)
    assert of_cells[0] == kv.fixed_mul(sum(c * l for c, l in zip(columns[0], l_at))) and nm.from_cells(as_coeff[2].cpu().numpy()) == [CONSTANT] + [0] * (N - 1)
    # the other way round: the same columns read as coefficients (X^700 among them, and the polynomial c (1 + X + ... + X^(n-1)))
    as_cells = ctx.coeff_to_lagrange(d_cells, K, tables, out=new("lagrange"))
    arena.check()
    of_coeff = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, d_cells.cpu().numpy(), bases["tau"], slices))
    of_cells = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, as_cells.cpu().numpy(), bases["lagrange"], slices))
    assert of_coeff == of_cells == [kv.commit(c) for c in columns] and of_coeff[1] == kv.tau_basis(K, TAU)[ROW]
    G.assert_bytes("the columns are left alone", d_cells.cpu().numpy(), cells(columns))


@pytest.mark.parametrize("x", (nm.seeded_values(1, 0x6b7a78)[0], 0, nm.omega(K)), ids=("seeded", "0", "omega"))
def test_one_opening_verifies_and_a_moved_evaluation_does_not(pkg, ctx, bases, x):
    columns = [nm.seeded_values(N, 0x6b7a50 + j) for j in range(2)]
    arena = G.DeviceArena(G.CANARIES[x % 2])
    d_coeff = put(arena, "coeff", cells(columns))
    ws = arena.out("ws", int(pkg.api.load_open_library().aesw_open_workspace_bytes(K, 2, 1)))
    quot, rem = ctx.divide_columns(d_coeff, K, x, out=arena.out("quot", 2 * N * 32, (2, N, 32)), _rem=arena.out("rem", 64, (2, 32)), _workspace=ws)
    arena.check()
    C = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, d_coeff.cpu().numpy(), bases["tau"], 0))
    W = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, quot.cpu().numpy(), bases["tau"], 0))
    e = nm.from_cells(rem.cpu().numpy())
    assert e == [kv.evaluate(c, x) for c in columns] and e[0] != e[1]
    for j in range(2):
        assert kv.verify_single(C[j], x, e[j], W[j], TAU), j
        assert not kv.verify_single(C[j], x, (e[j] + 1) % R, W[j], TAU) and not kv.verify_single(C[j], x, e[j], W[1 - j], TAU), j
    assert not kv.verify_single(C[0], (x + 1) % R, e[0], W[0], TAU)


# ---- the whole stage from its bytes -----------------------------------------------------------------------------------------------------

def prove(pkg, ctx, bases, canary, bump=None):
    """the device's proof of a stage over seeded columns: (plan, proof bytes, report, the columns' commitments as the device made them)"""
    import torch
    api = pkg.api
    plan = api.multiopen_plan(QUERIES)
    assert plan.rotations == list(sc.CHAIN_ROTATIONS) and plan.sets == [((0,), ["advice"]), ((0, 1), ["z"]), ((0, 1, 2), ["z2", "advice2"])]
    values = [[nm.seeded_values(N, 0x6b7a60 + 16 * i + j) for j in range(len(cols))] for i, (_idx, cols) in enumerate(plan.sets)]
    arena = G.DeviceArena(canary)
    columns = [put(arena, "columns%d" % i, cells(of_set)) for i, of_set in enumerate(values)]
    n_cols, n_evals = sum(plan.set_cols), len(plan.eval_order())
    capacity = 32 * (n_cols + n_evals + 2)
    t = ctx.transcript(capacity, _state=arena.out("state", 256), _proof=arena.out("proof", capacity))
    ws = arena.out("msm_ws", int(api.load_msm_library().aesw_msm_workspace_bytes(K, n_cols, mc.FR, 0)))
    commitments = ctx.commit_columns(torch.cat(columns), bases["tau"], out=arena.out("commitments", 64 * n_cols, (n_cols, 64)), _workspace=ws)
    t.write_points(commitments)
    x = nm.from_cells(t.squeeze(out=arena.out("x", 32)).cpu().numpy())[0]
    points = api.rotated_points(x, K, plan.rotations)
    evals = []
    for i, (idx, cols) in enumerate(plan.sets):  # column by column, point by point: the plan's order
        open_ws = arena.out("open_ws", int(api.load_open_library().aesw_open_workspace_bytes(K, len(cols), len(idx))))
        out = arena.out("evals%d" % i, 32 * len(cols) * len(idx), (len(cols), len(idx), 32))
        evals += nm.from_cells(ctx.evaluate_columns(columns[i], K, points[list(idx)], out=out, _workspace=open_ws).cpu().numpy())
    assert len(evals) == n_evals
    if bump is not None:
        evals[bump] = (evals[bump] + 1) % R
    d_evals = put(arena, "evals", nm.to_cells(evals))
    t.write_scalars(d_evals)
    out, report = ctx.open_shplonk(plan, columns, d_evals, put(arena, "points", points), t, bases["tau"], out=arena.out("out", 128, (2, 64)),
                                   _report=arena.out("report", 64).view(torch.int64))
    proof = t.proof()
    arena.check()
    assert t.status() == dict(proof_bytes=capacity, proof_missed=0, identities=0, first_identity=None)
    made = points_of(pkg, commitments.cpu().numpy())
    assert made == [kv.commit(c) for of_set in values for c in of_set]
    return plan, proof, api.shplonk_report_dict(report), made + points_of(pkg, out.cpu().numpy())


def test_the_verifier_accepts_the_devices_stage_from_its_bytes_alone(pkg, ctx, bases):
    plan, proof, report, points = prove(pkg, ctx, bases, G.CANARIES[0])
    assert report == dict(bad_sets=0, first_bad_set=None, zero_differences=0, z0_zero=0, last_remainder=[0, 0, 0, 0])
    verdict, read = kv.verify_proof(proof, plan, K, TAU)  # the bytes, the plan, and nothing else
    assert verdict, verdict
    assert read["points"] == points and None not in points and len(set(points)) == 6  # what the bytes say is what the device held
    assert len(set(read["challenges"].values())) == 4


def test_the_verifier_rejects_the_bytes_of_a_stage_with_one_evaluation_raised_by_1(pkg, ctx, bases):
    bump = 4  # eval_order()[4]: z2 at rotation 1, in set 2
    plan, proof, report, _points = prove(pkg, ctx, bases, G.CANARIES[1], bump=bump)
    assert plan.eval_order()[bump] == ("z2", 1)
    assert report["bad_sets"] == 1 and report["first_bad_set"] == 2 and report["z0_zero"] == 0 and any(report["last_remainder"])
    verdict, _read = kv.verify_proof(proof, plan, K, TAU)
    assert not verdict and verdict.reason == "equation"


# ---- at the kernels' extents ------------------------------------------------------------------------------------------------------------

def test_the_verifier_accepts_the_full_plan_as_the_device_opens_it(pkg, ctx, bases):
    import torch
    stage = sc.full_stage()
    p, pts, columns, evals, y, v, u = stage
    assert len(p.sets) == len(pts) == 16 and max(p.set_cols) == sc.WIDE_COLS == 257 and sum(p.set_cols) == 274
    got = run_stage(pkg, ctx, K, G.CANARIES[1], stage=stage)
    arena = got["arena"]
    ws = arena.out("divide_ws", int(pkg.api.load_open_library().aesw_open_workspace_bytes(K, 1, 1)))
    w, rem = ctx.divide_columns(got["line"], K, u, out=arena.out("w", N * 32, (N, 32)), _rem=arena.out("last", 32), _workspace=ws)
    arena.check()
    assert not rem.cpu().numpy().any() and pkg.api.shplonk_report_dict(got["report"])["bad_sets"] == 0
    H, W = points_of(pkg, commit(pkg, ctx, arena, mc.FR, K, torch.stack([got["h"], w]).cpu().numpy(), bases["tau"], 0))
    commitments = [[kv.commit(c) for c in of_set] for of_set in columns]  # by their exponents: the multi-scalar product is held above
    verdict = kv.verify_shplonk(p, commitments, evals, pts, y, v, u, H, W, TAU)
    assert verdict, verdict
    assert kv.verify_shplonk(p, commitments, evals, pts, y, v, u, W, H, TAU).reason == "equation" and H != W and None not in (H, W)
