"""The transforms over real columns on the GPU, on the shape of tests/test_gpu_grand_chain.py: a FixedAes128Config<17, 2> circuit of
150 blocks.  The columns are one lookup Z from Context.grand_product (its blinding rows zero) and one advice column assembled as
Fr cells.  lagrange_to_coeff of both and coeff_to_lagrange back gives the columns bit for bit; evaluate of the advice coefficients
at omega^i gives the witness byte at 64 rows; coeff_to_extended with ext_k = 19 agrees with evaluate at 16 seeded coset points;
extended_to_coeff returns the 2^17 coefficients and 3 * 2^17 zero cells.  The five calls -- the tables and the four transforms --
are captured in one graph and replayed twice after the input column is overwritten: the outputs follow the input."""
import numpy as np
import pytest

import grand_cases as gc
import ntt_cases as nc
import ntt_model as nm

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N, EXT_K = nc.CHAIN
U = (1 << K) - 6
THETA = gc.seeded(gc.THETA_SEED)
BETA, GAMMA = (gc.seeded(s) for s in gc.CHALLENGE_SEEDS)


@pytest.fixture(scope="module")
def chain(pkg, ctx):
    import torch
    rng = np.random.default_rng(0x6e7463)
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
    columns = torch.stack([z[1, 2], advice_fr[4]]).contiguous()  # a Z of the second set; y of the second set
    tables = ctx.ntt_tables(EXT_K)
    coeff = ctx.lagrange_to_coeff(columns, K, tables)
    torch.cuda.synchronize()
    return dict(columns=columns, bytes=advice_bytes[4].cpu().numpy(), tables=tables, coeff=coeff, advice_coeff=nm.from_cells(coeff[1].cpu().numpy()))


def test_to_coefficients_and_back_gives_the_columns_bit_for_bit(ctx, chain):
    import torch
    c = chain
    assert c["columns"][0, :U + 1].any() and c["bytes"].any()
    back = ctx.coeff_to_lagrange(c["coeff"], K, c["tables"])
    assert torch.equal(back, c["columns"])
    assert not torch.equal(c["coeff"], c["columns"])


def test_the_advice_polynomial_takes_the_witness_bytes_on_the_domain(chain):
    c = chain
    w = nm.omega(K)
    rows = [0, (1 << K) - 1] + [int(v) for v in np.random.default_rng(0x6164).integers(0, U, 62)]
    assert [nm.evaluate(c["advice_coeff"], pow(w, i, nm.R)) for i in rows] == [int(c["bytes"][i]) for i in rows]
    assert len({int(c["bytes"][i]) for i in rows}) > 8


def test_the_extended_column_is_the_polynomial_on_the_coset_and_comes_back_padded(ctx, chain):
    import torch
    c = chain
    ext = ctx.coeff_to_extended(c["coeff"], K, EXT_K, c["tables"], zeta_sel=1)
    rows = [int(v) for v in np.random.default_rng(0x6578).integers(0, 1 << EXT_K, 16)]
    got = nm.from_cells(ext[1][rows].cpu().numpy())
    w = nm.omega(EXT_K)
    assert got == [nm.evaluate(c["advice_coeff"], nm.ZETAS[1] * pow(w, j, nm.R) % nm.R) for j in rows]
    back = ctx.extended_to_coeff(ext, EXT_K, c["tables"], zeta_sel=1)
    assert torch.equal(back[:, :1 << K], c["coeff"]) and not back[:, 1 << K:].any() and back.shape[1] == 4 << K


def test_the_captured_calls_follow_the_input_column_through_two_replays(pkg, ctx, chain):
    import torch
    c = chain
    lib = pkg.api.load_ntt_library()
    poison = 0xA5
    dev = c["columns"].device
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device=dev)  # noqa: E731
    column = c["columns"][:1].clone()
    tables = full(int(lib.aesw_ntt_tables_bytes(EXT_K)) // 32, 32)
    coeff, back, ext, ext_coeff = full(1, 1 << K, 32), full(1, 1 << K, 32), full(1, 1 << EXT_K, 32), full(1, 1 << EXT_K, 32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ctx.ntt_tables(EXT_K, _out=tables)
        ctx.lagrange_to_coeff(column, K, tables, out=coeff)
        ctx.coeff_to_lagrange(coeff, K, tables, out=back)
        ctx.coeff_to_extended(coeff, K, EXT_K, tables, zeta_sel=1, out=ext)
        ctx.extended_to_coeff(ext, EXT_K, tables, zeta_sel=1, out=ext_coeff)
    torch.cuda.synchronize()
    assert bool((ext_coeff == poison).all()) and bool((tables == poison).all()), "the captured calls ran during capture"
    for which in (0, 1):
        column.copy_(c["columns"][which:which + 1])
        for t in (coeff, back, ext, ext_coeff):
            t.fill_(poison)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tables, c["tables"])
        assert torch.equal(coeff, c["coeff"][which:which + 1]) and torch.equal(back, column), which
        assert torch.equal(ext_coeff[:, :1 << K], coeff) and not ext_coeff[:, 1 << K:].any(), which
        if which == 1:  # the advice column: the replayed extension is the polynomial on the coset
            rows = [0, (1 << EXT_K) - 1, 12345, 1 << K]
            w = nm.omega(EXT_K)
            assert nm.from_cells(ext[0][rows].cpu().numpy()) == [nm.evaluate(c["advice_coeff"], nm.ZETAS[1] * pow(w, j, nm.R) % nm.R) for j in rows]
