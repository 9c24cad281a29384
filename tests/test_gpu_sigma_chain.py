"""The permutation argument on the GPU from a real witness: a FixedAes128Config<17, 2> circuit of 150 blocks (the shape of
tests/test_gpu_grand_chain.py) -- byte columns from assemble_advice, the fixed round-constant column from selector_tags(),
permutation_mapping, then the product with chunk_len 3 over the 8 columns (3 sets).  The last closing cell is the Montgomery one.
At some hundred seeded rows, the set boundaries among them, Z[i + 1] * den[i] = Z[i] * num[i] and Z_{s+1}[0] = Z_s[n_rows], with num
and den from tests/sigma_model.py for those rows only.  One corrupted byte in a copy destination opens the argument; one in a cell
no copy touches leaves it closed.  The product captured into a graph follows the beta cell through two replays."""
import numpy as np
import pytest

import sigma_cases as sc
import sigma_model as sm

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N, CHUNK_LEN = sc.CHAIN
U = (1 << K) - 6
BETA, GAMMA = (sc.seeded(s) for s in sc.CHALLENGE_SEEDS)
BETA_2 = sc.seeded(0x7332)
CLOSED = {"sets": 3, "open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}


@pytest.fixture(scope="module")
def chain(pkg, ctx):
    import torch
    assert N < pkg.block_capacity(K, N_SETS) and pkg.api.block_placement(K, N_SETS, N - 1)[0] == 1  # both sets hold blocks
    for b in (0, N - 1):
        assert pkg.api.block_placement(K, N_SETS, b)[1] + pkg.AES_ROWS <= U
    rng = np.random.default_rng(0x7369676d61)
    d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    d_pt = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    advice = ctx.assemble_advice(K, N_SETS, w, kw, N, layout=PACKED)
    fixed = np.zeros((1, 1 << K), np.uint8)
    fixed[0, :96] = pkg.selector_tags()[3]  # the round constants, in the rows of words_column
    mapping = pkg.api.permutation_mapping(K, N_SETS, N)
    n_cols = pkg.api.permutation_columns(N_SETS)
    assert n_cols == 8 and mapping.shape == (8, 1 << K)
    buffers = np.concatenate([advice.cpu().numpy(), fixed])
    return dict(advice=advice, fixed=torch.from_numpy(fixed).cuda(), source=pkg.api.permutation_sources(N_SETS), mapping=mapping,
                d_mapping=torch.from_numpy(mapping.view(np.int32)).cuda(), tables=ctx.permutation_tables(K, n_cols), n_cols=n_cols,
                columns=[buffers[s] for s in sm.sources(N_SETS)])


def run(ctx, c, advice=None, beta=BETA, **kw):
    return ctx.permutation_product(K, c["n_cols"], CHUNK_LEN, c["advice"] if advice is None else advice, c["fixed"], c["source"], c["d_mapping"], c["tables"],
                                   beta, GAMMA, n_rows=U, **kw)


def recurrence_holds(c, z, closing, beta):
    rng = np.random.default_rng(0x726f7773)
    rows = sorted({0, 1, 399, 400, 1023, 1024, U - 2, U - 1} | {int(i) for i in rng.integers(0, U, 120)})
    terms = sm.row_terms(K, c["columns"], c["mapping"], beta, GAMMA, CHUNK_LEN, rows)
    z = z.cpu()
    for s, (nums, dens) in enumerate(terms):
        here, after = sm.values(z[s, rows].numpy()), sm.values(z[s, [i + 1 for i in rows]].numpy())
        for i, zi, zn, num, den in zip(rows, here, after, nums, dens):
            assert zn * den % sm.R == zi * num % sm.R and den and zi, (s, i)
        first, last = sm.values(z[s, [0, U]].numpy())
        assert last == sm.values(closing[s].cpu().numpy())[0]
        assert first == (1 if s == 0 else sm.values(closing[s - 1].cpu().numpy())[0]), s  # halo2's last_z
    assert any(num != den for nums, dens in terms for num, den in zip(nums, dens))  # the sampled rows hold copies: Z is no constant column


def test_the_argument_closes_and_z_obeys_the_recurrence(pkg, ctx, chain):
    z, closing, rep = run(ctx, chain)
    assert rep == CLOSED
    assert bytes(closing[-1].cpu().numpy()) == sm.ONE_CELL and bytes(z[0, 0].cpu().numpy()) == sm.ONE_CELL
    recurrence_holds(chain, z, closing, BETA)
    assert len({bytes(v) for v in closing.cpu().numpy()}) == 3  # every set moves Z: the chain across sets is no chain of ones


def test_a_corrupted_copy_destination_opens_it_and_a_cell_no_copy_touches_does_not(pkg, ctx, chain):
    c = chain
    first = pkg.api.block_placement(K, N_SETS, 3)[1]
    col, row = next((col, i) for col in (0, 1, 2) for i in range(first, first + pkg.AES_ROWS) if c["mapping"][col, i] != (col << K) + i)
    advice = c["advice"].clone()
    advice[int(c["source"][col]), row] ^= 0x10
    _z, closing, rep = run(ctx, c, advice=advice)
    assert rep == dict(CLOSED, open=True) and bytes(closing[-1].cpu().numpy()) != sm.ONE_CELL
    # a row behind the last block of set 1 (columns 5 ... 7): assigned by nobody, copied by nobody
    free_row = pkg.api.block_placement(K, N_SETS, N - 1)[1] + 2 * pkg.AES_ROWS
    assert free_row < U and c["mapping"][5, free_row] == (5 << K) + free_row
    advice = c["advice"].clone()
    advice[int(c["source"][5]), free_row] ^= 0x10
    _z, closing, rep = run(ctx, c, advice=advice)
    assert rep == CLOSED and bytes(closing[-1].cpu().numpy()) == sm.ONE_CELL


def test_the_captured_product_follows_the_beta_cell_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    lib = pkg.api.load_sigma_library()
    side = torch.cuda.Stream()
    workspace = torch.empty(int(lib.aesw_sigma_workspace_bytes(K, c["n_cols"], CHUNK_LEN)), dtype=torch.uint8, device="cuda")
    d_beta, d_gamma = torch.from_numpy(pkg.api.fr_cell(BETA)).cuda(), torch.from_numpy(pkg.api.fr_cell(GAMMA)).cuda()
    d_source = torch.from_numpy(c["source"].view(np.int32)).cuda()
    poison = 0xA5
    z = torch.full((3, 1 << K, 32), poison, dtype=torch.uint8, device="cuda")
    closing = torch.full((3, 32), poison, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _z, _c, rep = ctx.permutation_product(K, c["n_cols"], CHUNK_LEN, c["advice"], c["fixed"], d_source, c["d_mapping"], c["tables"], d_beta, d_gamma, n_rows=U,
                                              sync=False, _out=(z, closing), _workspace=workspace)
    torch.cuda.synchronize()
    assert bool((z == poison).all()) and bool((closing == poison).all()), "the captured call ran during capture"
    seen = []
    for beta in (BETA, BETA_2):
        d_beta.copy_(torch.from_numpy(pkg.api.fr_cell(beta)).cuda())
        z.fill_(poison)
        closing.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert pkg.api.sigma_report_dict(rep) == CLOSED, beta
        recurrence_holds(c, z, closing, beta)
        assert bool((z[:, U + 1:] == poison).all())
        seen.append(bytes(z[0, 1000].cpu().numpy()))
    assert seen[0] != seen[1]  # the two betas give different columns
