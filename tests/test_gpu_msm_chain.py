"""Commitments over real columns on the GPU, on the shape of tests/test_gpu_open_chain.py: a FixedAes128Config<17, 2> circuit of 150
blocks.  The basis is the model's basis of known logarithms at 2^10 points, tiled to the 2^17 rows (every point on the curve; the
logarithm of row i is that of point i mod 1024), so an expectation stays one scalar multiplication.  An assembled advice column is
committed as bytes and as the same values in Fr cells: one point, and the model's.  Linearity on the device: commit(a) +
commit(b), summed in the model, is commit(a + b).  The call is captured in one linear graph on a side stream and replayed twice
with the scalars changed in between: the commitment follows them, and nothing ran during capture."""
import numpy as np
import pytest

import msm_cases as mc
import msm_model as mm

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N = 17, 2, 150
TILE_K = 10


def tiled_commit(values):
    """the commitment of 2^K values against the tiled basis, by the logarithms"""
    folded = np.asarray(values, dtype=object).reshape(-1, 1 << TILE_K).sum(axis=0)
    return mm.known_commit([int(v) for v in folded])


@pytest.fixture(scope="module")
def chain(pkg, ctx):
    import torch
    rng = np.random.default_rng(0x6d736d)
    d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    d_pt = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    advice_bytes = ctx.assemble_advice(K, N_SETS, w, kw, N, PACKED)
    advice_fr = ctx.assemble_advice(K, N_SETS, w, kw, N, PACKED, as_fr=True)
    basis = torch.from_numpy(np.tile(mc.basis_cells(TILE_K), (1 << (K - TILE_K), 1))).cuda()
    torch.cuda.synchronize()
    return dict(bytes=advice_bytes, fr=advice_fr, basis=basis)


def test_an_advice_column_commits_to_one_point_as_bytes_and_as_cells(pkg, ctx, chain):
    import torch
    c = chain
    columns = [3, 4]  # x and y of the second set
    as_bytes = ctx.commit_columns(c["bytes"][columns].contiguous(), c["basis"])
    as_cells = ctx.commit_columns(c["fr"][columns].contiguous(), c["basis"])
    assert tuple(as_bytes.shape) == (2, 64) and torch.equal(as_bytes, as_cells)
    host = c["bytes"][columns].cpu().numpy()
    assert len(np.unique(host[1])) > 16  # a real column, not one value throughout
    assert pkg.api.g1_from_cells(as_bytes.cpu().numpy()) == [tiled_commit(col) for col in host]


def test_commitments_are_linear_on_the_device(pkg, ctx, chain):
    import torch
    c = chain
    a, b = (mm.seeded_scalars(1 << K, s) for s in (0x6c61, 0x6c62))
    total = [(x + y) % mm.R for x, y in zip(a, b)]
    cells = torch.from_numpy(np.stack([mm.scalar_cells(v) for v in (a, b, total)])).cuda()
    p_a, p_b, p_total = pkg.api.g1_from_cells(ctx.commit_columns(cells, c["basis"]).cpu().numpy())
    assert mm.add(p_a, p_b) == p_total and p_a != p_b and None not in (p_a, p_b, p_total)
    assert p_a == tiled_commit(a)


def test_a_captured_call_follows_the_scalars_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    lib = pkg.api.load_msm_library()
    poison = 0xA5
    dev = c["basis"].device
    scalars = c["bytes"][3:5].contiguous().clone()
    out = torch.full((2, 64), poison, dtype=torch.uint8, device=dev)
    ws = torch.full((int(lib.aesw_msm_workspace_bytes(K, 2, mc.BYTES, 0)),), poison, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.commit_columns(scalars, c["basis"], out=out, _workspace=ws)
    torch.cuda.synchronize()
    assert bool((out == poison).all()) and bool((ws == poison).all()), "the captured call ran during capture"
    rng = np.random.default_rng(0x7265706c)
    for _ in range(2):
        host = rng.integers(0, 256, (2, 1 << K), dtype=np.uint8)
        scalars.copy_(torch.from_numpy(host).to(dev))
        out.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert pkg.api.g1_from_cells(out.cpu().numpy()) == [tiled_commit(col) for col in host]
