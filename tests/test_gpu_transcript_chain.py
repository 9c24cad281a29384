"""Challenges from commitments without a host in between, on the GPU: at k = 10 three byte columns are committed
(Context.commit_columns), the tensor of commitments goes straight to Transcript.write_points, the tensor squeeze() returns goes
straight to compress_table as theta, the next two to invert_table as beta and gamma.  The tables equal, byte for byte, those of the
same calls given the model's challenges (tests/transcript_model.py over the commitments read back) as Python ints.  Then the
linear chain init -> write_points -> squeeze -> compress_table is captured on one stream, with no parallel branch, and replayed
twice with the commitments changed in between: each replay's table is the one of its own commitments, and the proof bytes and
the cursor are the model's after each."""
import numpy as np
import pytest

import msm_cases as mc
import transcript_model as tm

pytestmark = pytest.mark.gpu
K, COLUMNS = 10, ("seeded", "ends", "seeded2")


@pytest.fixture(scope="module")
def chain(pkg, ctx):
    import torch
    basis = torch.from_numpy(mc.basis_cells(K)).cuda()
    columns = torch.from_numpy(np.stack([np.array(mc.byte_columns(K)[name], np.uint8) for name in COLUMNS])).cuda()
    commitments = ctx.commit_columns(columns, basis)
    torch.cuda.synchronize()
    return dict(basis=basis, columns=columns, commitments=commitments)


def model_of(pkg, commitments, squeezes):
    """(the model's transcript after write_points of the commitments, its first `squeezes` challenges)"""
    points = pkg.api.g1_from_cells(commitments.cpu().numpy())
    t = tm.Transcript().write_points(points)
    return t, [t.squeeze() for _ in range(squeezes)]


def test_the_commitments_give_theta_beta_and_gamma_on_the_device(pkg, ctx, chain):
    import torch
    c = chain
    assert c["commitments"].cpu().numpy().tobytes() == b"".join(mc.expected(mc.BYTES, K, name).tobytes() for name in COLUMNS)
    t = ctx.transcript(len(COLUMNS) * 32)
    theta = t.write_points(c["commitments"]).squeeze()
    beta, gamma = t.squeeze(), t.squeeze()
    table, rep = ctx.compress_table(theta)
    inv, inv_rep = ctx.invert_table(table, beta, gamma)
    model, (m_theta, m_beta, m_gamma) = model_of(pkg, c["commitments"], 3)
    assert [x.cpu().numpy().tobytes() for x in (theta, beta, gamma)] == [tm.challenge_cell(v).tobytes() for v in (m_theta, m_beta, m_gamma)]
    assert len({m_theta, m_beta, m_gamma}) == 3 and not rep["noncanonical"]
    table_ints, _ = ctx.compress_table(m_theta)
    inv_ints, _ = ctx.invert_table(table_ints, m_beta, m_gamma)
    assert torch.equal(table, table_ints) and torch.equal(inv, inv_ints) and bool(table.any()) and bool(inv.any())
    assert t.proof() == model.proof and len(model.proof) == 96
    assert t.status() == model.status(96)


def test_the_captured_chain_follows_the_commitments_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    poison = 0xA5
    dev = c["basis"].device
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device=dev)  # noqa: E731
    commitments = c["commitments"].clone()
    state, proof, theta, table = full(tm.STATE_BYTES), full(len(COLUMNS) * 32), full(32), full(*pkg.api.TABLE_FR_SHAPE)
    t = ctx.transcript(len(COLUMNS) * 32, _state=state, _proof=proof)
    torch.cuda.synchronize()
    state.fill_(poison)  # the constructor's init is not the chain's
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        t.reset()
        t.write_points(commitments)
        t.squeeze(out=theta)
        _table, report = ctx.compress_table(theta, sync=False, _out=table)
    torch.cuda.synchronize()
    assert all(bool((x == poison).all()) for x in (state, proof, theta, table)), "the captured calls ran during capture"
    other = ctx.commit_columns(c["columns"].flip(0).contiguous(), c["basis"])  # the same three points in another order
    torch.cuda.synchronize()
    seen = []
    for source in (c["commitments"], other):
        commitments.copy_(source)
        for x in (proof, theta, table):
            x.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        model, (m_theta,) = model_of(pkg, source, 1)
        assert theta.cpu().numpy().tobytes() == tm.challenge_cell(m_theta).tobytes()
        expected, _ = ctx.compress_table(m_theta)
        assert torch.equal(table, expected)
        assert t.proof() == model.proof and t.status() == model.status(96)  # init is in the chain: the cursor starts at 0 in every replay
        seen.append(m_theta)
    assert seen[0] != seen[1] and report is not None
