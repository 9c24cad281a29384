"""Evaluation, fold and division over real columns on the GPU, on the shape of tests/test_gpu_ntt_chain.py: a FixedAes128Config<17, 2>
circuit of 150 blocks (oc.CHAIN).  The columns are one lookup Z from Context.grand_product (its blinding rows zero) and one advice
column assembled as Fr cells, both brought to coefficient form by lagrange_to_coeff.  The advice polynomial evaluated on the device
at rotated_points(1, K, rows) gives the witness bytes at eight seeded rows; the quotient of a division at a seeded x, evaluated at y,
satisfies p(y) - p(x) == q(y) (y - x); the evaluation at x of the fold of the two columns under v is the fold of their two
evaluations.  The three calls are captured in one linear graph on a side stream and replayed twice after the point's cell is
overwritten: the outputs follow the point, and nothing ran during capture."""
import numpy as np
import pytest

import grand_cases as gc
import ntt_model as nm
import open_cases as oc
import open_model as om

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N = oc.CHAIN
U = (1 << K) - 6
THETA = gc.seeded(gc.THETA_SEED)
BETA, GAMMA = (gc.seeded(s) for s in gc.CHALLENGE_SEEDS)
X, Y, V = nm.seeded_values(3, 0x6f7063)


@pytest.fixture(scope="module")
def chain(pkg, ctx):
    import torch
    rng = np.random.default_rng(0x6f7063)
    d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    d_pt = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    mult, rep = ctx.lookup_multiplicities(K, N_SETS, w, kw, [N], PACKED)
    assert rep["misses"] == 0
    a, s, _prep = ctx.permuted_columns(K, N_SETS, mult, n_rows=U, pad_row=0)
    inputs, _irep = ctx.lookup_inputs(K, N_SETS, w, kw)
    table, _trep = ctx.compress_table(THETA)
    inv, _vrep = ctx.invert_table(table, BETA, GAMMA)
    z = torch.zeros((N_SETS, 5, 1 << K, 32), dtype=torch.uint8, device="cuda")  # the blinding rows: zero, canonical
    closing = torch.zeros((N_SETS, 5, 32), dtype=torch.uint8, device="cuda")
    _z, _c, grep = ctx.grand_product(K, N_SETS, inputs, a, s, table, inv, BETA, GAMMA, n_rows=U, _out=(z, closing))
    assert grep["open"] == 0
    advice_bytes = ctx.assemble_advice(K, N_SETS, w, kw, N, PACKED)
    advice_fr = ctx.assemble_advice(K, N_SETS, w, kw, N, PACKED, as_fr=True)
    columns = torch.stack([advice_fr[4], z[1, 2]]).contiguous()  # y of the second set; a Z of the second set
    coeff = ctx.lagrange_to_coeff(columns, K, ctx.ntt_tables(K))
    torch.cuda.synchronize()
    return dict(bytes=advice_bytes[4].cpu().numpy(), coeff=coeff, values=[nm.from_cells(c.cpu().numpy()) for c in coeff])


def test_the_advice_polynomial_takes_the_witness_bytes_at_the_rotated_points(pkg, ctx, chain):
    c = chain
    # eight rows: the first, the last usable one, and six seeded ones among the rows the 150 blocks assign (most rows of y are 0)
    assigned = np.nonzero(c["bytes"])[0]
    rows = [0, U - 1] + [int(assigned[v]) for v in np.random.default_rng(0x726f).integers(0, len(assigned), 6)]
    points = pkg.api.rotated_points(1, K, rows)  # omega^row: the domain's own points
    got = ctx.evaluate_columns(c["coeff"][0], K, points)
    assert tuple(got.shape) == (len(rows), 32)
    assert nm.from_cells(got.cpu().numpy()) == [int(c["bytes"][i]) for i in rows]
    assert len({int(c["bytes"][i]) for i in rows}) > 2  # not one value throughout


def test_the_quotient_of_a_division_satisfies_the_identity_at_a_second_point(ctx, chain):
    c = chain
    quot, rem = ctx.divide_columns(c["coeff"], K, X)
    p_y, q_y = ctx.evaluate_columns(c["coeff"], K, [Y]), ctx.evaluate_columns(quot, K, [Y])
    p_x, p_y, q_y = (nm.from_cells(t.cpu().numpy()) for t in (rem, p_y, q_y))
    assert p_x == [nm.evaluate(v, X) for v in c["values"]] and p_x[0] != p_x[1]
    assert [(a - b) % nm.R for a, b in zip(p_y, p_x)] == [q * (Y - X) % nm.R for q in q_y]
    assert not quot[:, -1].any() and quot[:, -2].any()


def test_the_evaluation_of_a_fold_is_the_fold_of_the_evaluations(ctx, chain):
    c = chain
    folded = ctx.fold_columns(c["coeff"], K, V)
    at_x = nm.from_cells(ctx.evaluate_columns(folded, K, [X]).cpu().numpy())
    advice_x, z_x = nm.from_cells(ctx.evaluate_columns(c["coeff"], K, [X]).cpu().numpy())
    assert at_x == [(advice_x * V + z_x) % nm.R] and advice_x and z_x


def test_the_captured_calls_follow_the_point_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    lib = pkg.api.load_open_library()
    poison = 0xA5
    coeff = c["coeff"]
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device=coeff.device)  # noqa: E731
    point = torch.from_numpy(pkg.api.fr_cell(X)).to(coeff.device).view(1, 32)
    evals, folded, quot, rem = full(2, 1, 32), full(1 << K, 32), full(2, 1 << K, 32), full(2, 32)
    ws_evaluate, ws_divide = (full(int(lib.aesw_open_workspace_bytes(K, 2, 1))) for _ in range(2))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.evaluate_columns(coeff, K, point, out=evals, _workspace=ws_evaluate)
        ctx.fold_columns(coeff, K, point, out=folded)
        ctx.divide_columns(coeff, K, point, out=quot, _rem=rem, _workspace=ws_divide)
    torch.cuda.synchronize()
    for t in (evals, folded, quot, rem, ws_evaluate, ws_divide):
        assert bool((t == poison).all()), "the captured calls ran during capture"
    for x in (Y, V):  # neither is the point the capture saw
        point.copy_(torch.from_numpy(pkg.api.fr_cell(x)).to(coeff.device).view(1, 32))
        for t in (evals, folded, quot, rem):
            t.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expected = [om.divide(v, x) for v in c["values"]]
        assert nm.from_cells(evals.cpu().numpy()) == [r for _q, r in expected] == nm.from_cells(rem.cpu().numpy()), x
        assert np.array_equal(quot.cpu().numpy(), np.stack([nm.to_cells(q) for q, _r in expected])), x
        assert np.array_equal(folded.cpu().numpy(), nm.to_cells(om.fold(c["values"], x))), x
