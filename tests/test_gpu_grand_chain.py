"""The whole device chain on the GPU, from a real witness to Z: a FixedAes128Config<17, 2> circuit of 150 blocks -- such a circuit
holds 191, so "a few hundred" is 150 here: both sets hold blocks, the second is partly filled, and every block row lies below
n_rows = 2^17 - 6 -- through the multiplicities, the permuted columns, the input column, the compression under
theta, the inverse table and the grand product.  A' and S' permute A and S over the usable rows, so every closing cell is the
Montgomery one and no argument is open; Z equals tests/grand_model.py's.  One corrupted word of d_a opens exactly that argument.
The part of the chain a prover repeats per challenge -- the input column, the compression under theta, the inverse table and the
grand product -- is captured once into a graph with the workspaces prepared beforehand and replayed twice with the beta cell
rewritten in between: both replays equal the model for their beta.  The multiplicities and the permuted columns stay outside
the capture: they need no challenge, their Python wrappers allocate and upload on the way (the block offsets, the workspace),
which a capture does not allow, and their own capture tests are tests/test_gpu_mult.py's and tests/test_gpu_perm.py's."""
import numpy as np
import pytest

import grand_cases as gc
import grand_model as gm
import theta_model as tm

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N = gc.K, 2, 150
U = (1 << K) - 6
THETA = gc.seeded(gc.THETA_SEED)
BETA, GAMMA = (gc.seeded(s) for s in gc.CHALLENGE_SEEDS)
BETA_2 = gc.seeded(0x6232)


@pytest.fixture(scope="module")
def chain(pkg, ctx, oracle):
    import torch
    assert N < pkg.block_capacity(K, N_SETS)
    for b in (0, N - 1):
        assert pkg.api.block_placement(K, N_SETS, b)[1] + pkg.AES_ROWS <= U
    assert pkg.api.block_placement(K, N_SETS, N - 1)[0] == 1  # both sets hold blocks
    rng = np.random.default_rng(0x636861696e)
    d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    d_pt = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    mult, rep = ctx.lookup_multiplicities(K, N_SETS, w, kw, [N], PACKED)
    assert rep["misses"] == 0
    a, s, prep = ctx.permuted_columns(K, N_SETS, mult, n_rows=U, pad_row=0)
    assert prep["overflowed"] == 0
    inputs, irep = ctx.lookup_inputs(K, N_SETS, w, kw)
    assert irep == rep
    table, trep = ctx.compress_table(THETA)
    model_table = tm.compressed_tables(oracle.lookup_table(), THETA)
    assert not trep["noncanonical"] and np.array_equal(table.cpu().numpy(), model_table)
    host = [t.cpu().numpy() for t in (inputs, a, s)]
    return dict(w=w, kw=kw, inputs=inputs, a=a, s=s, table=table, model_table=model_table, host=host, z={})


def model(c, beta):
    if beta not in c["z"]:
        c["z"][beta] = gm.grand_product(c["model_table"], *c["host"], beta, GAMMA, 0, rows=U)
    return c["z"][beta]


def test_the_chain_closes_every_argument_and_z_is_the_models(pkg, ctx, chain):
    c = chain
    inv, rep = ctx.invert_table(c["table"], BETA, GAMMA)
    assert rep == {"cells": 2 * 3 * gm.BINS, "noncanonical": False, "zero_terms": 0}
    z, closing, rep = ctx.grand_product(K, N_SETS, c["inputs"], c["a"], c["s"], c["table"], inv, BETA, GAMMA, n_rows=U)
    assert rep == {"arguments": 10, "open": 0, "first_open": None}
    assert all(bytes(cell) == gm.ONE_CELL for cell in closing.cpu().numpy().reshape(-1, 32))
    exp_z, exp_closing = gm.z_cells(model(c, BETA), U, K)
    assert gm.report(model(c, BETA), U) == rep and np.array_equal(closing.cpu().numpy(), exp_closing)
    got = z[:, :, :U + 1].cpu().numpy()
    bad = np.argwhere((got != exp_z).any(axis=3))
    assert not bad.size, "%d cells of Z differ, first (set, tag - 1, row) %r" % (len(bad), bad[0].tolist())
    assert all(bytes(got[st, t, 0]) == gm.ONE_CELL and bytes(got[st, t, U]) == gm.ONE_CELL for st in range(N_SETS) for t in range(5))


def test_one_corrupted_word_of_a_opens_that_argument_alone(pkg, ctx, chain):
    c = chain
    inv, _ = ctx.invert_table(c["table"], BETA, GAMMA)
    st, tag, at = 1, 2, 12345
    a = c["a"].clone()
    a[st, tag - 1, at] = (int(a[st, tag - 1, at]) + 1) % gm.ZERO_ROW
    _z, closing, rep = ctx.grand_product(K, N_SETS, c["inputs"], a, c["s"], c["table"], inv, BETA, GAMMA, n_rows=U)
    assert rep == {"arguments": 10, "open": 1, "first_open": (st, tag)}
    cells = closing.cpu().numpy()
    assert [(s_, t) for s_ in range(N_SETS) for t in range(5) if bytes(cells[s_, t]) != gm.ONE_CELL] == [(st, tag - 1)]


def test_the_captured_chain_follows_the_beta_cell_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    lib = pkg.api.load_grand_library()
    side = torch.cuda.Stream()
    ctx.prepare_lookup_inputs(K, N_SETS, side)
    workspace = torch.empty(int(lib.aesw_grand_workspace_bytes(K, N_SETS)), dtype=torch.uint8, device="cuda")
    d_theta = torch.from_numpy(pkg.api.fr_cell(THETA)).cuda()
    d_beta, d_gamma = torch.from_numpy(pkg.api.fr_cell(BETA)).cuda(), torch.from_numpy(pkg.api.fr_cell(GAMMA)).cuda()
    poison = 0xA5
    inputs = torch.full_like(c["inputs"], -1)
    table = torch.full_like(c["table"], poison)
    inv = torch.full((2, 3, gm.BINS, 32), poison, dtype=torch.uint8, device="cuda")
    z = torch.full((N_SETS, 5, 1 << K, 32), poison, dtype=torch.uint8, device="cuda")
    closing = torch.full((N_SETS, 5, 32), poison, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _i, irep = ctx.lookup_inputs(K, N_SETS, c["w"], c["kw"], sync=False, _out=inputs)
        _t, trep = ctx.compress_table(d_theta, sync=False, _out=table)
        _v, vrep = ctx.invert_table(table, d_beta, d_gamma, sync=False, _out=inv)
        _z, _c, rep = ctx.grand_product(K, N_SETS, inputs, c["a"], c["s"], table, inv, d_beta, d_gamma, n_rows=U, sync=False, _out=(z, closing), _workspace=workspace)
    torch.cuda.synchronize()
    assert bool((z == poison).all()) and bool((closing == poison).all()), "the captured calls ran during capture"
    for beta in (BETA, BETA_2):
        d_beta.copy_(torch.from_numpy(pkg.api.fr_cell(beta)).cuda())
        z.fill_(poison)
        closing.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        exp_z, exp_closing = gm.z_cells(model(c, beta), U, K)
        assert pkg.api.grand_report_dict(rep) == {"arguments": 10, "open": 0, "first_open": None}, beta
        assert pkg.api.grand_invert_report_dict(vrep)["zero_terms"] == 0 and torch.equal(inputs, c["inputs"])
        assert np.array_equal(closing.cpu().numpy(), exp_closing) and np.array_equal(z[:, :, :U + 1].cpu().numpy(), exp_z), beta
        assert bool((z[:, :, U + 1:] == poison).all())
    assert model(c, BETA)[0][1][1000] != model(c, BETA_2)[0][1][1000]  # the two betas give different columns
