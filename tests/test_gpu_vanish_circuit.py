"""The quotient of a real circuit on the GPU: the device-made column groups of tests/test_gpu_argument_rows.py's shape (17, 2, 150, 3)
-- one key, 150 plaintexts, every prover stage on the device -- blinded above n_rows as a prover blinds them, taken through
lagrange_to_coeff, coeff_to_extended (ext_k = 19), the accumulator of libaesw_vanish.so and extended_to_coeff.  On seeded columns
the numerator is not divisible by x^n - 1; here it is, so h is a polynomial and the identity of the vanishing argument holds at a
point off the coset:  fold(quot_model.constraints at x) = h(x) * (x^n - 1),  every column's value at x, x omega, x / omega and
x omega^n_rows from evaluate_columns.  After one flipped byte of a copied advice cell the identity fails.  The pieces of
quotient_pieces sum back to h:  sum_i x^(n i) h_i(x) = h(x)."""
import numpy as np
import pytest

import argument_rows as ar
import ntt_model as nm
import quot_model as qm
import sigma_cases as sc
import theta_model as tm

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, BLOCKS, CHUNK_LEN = sc.CHAIN
EXT_K, ZETA_SEL = K + 2, 1
N = 1 << K
U = N - 6
R = nm.R
THETA, BETA, GAMMA, Y, X = (sc.seeded(s) for s in (0x76637468, 0x76636265, 0x76636761, 0x76630079, 0x76630078))
ROTATIONS = (0, 1, -1, U)


def blind(t, first, seed):
    """rows first ... 2^k - 1 of every column of t [columns, 2^k, 32]: seeded canonical cells, as a prover blinds them"""
    import torch
    tail = N - first
    cells = nm.to_cells(nm.seeded_values(t.shape[0] * tail, seed)).reshape(t.shape[0], tail, 32)
    t[:, first:] = torch.from_numpy(cells).to(t.device)
    return t


@pytest.fixture(scope="module")
def lagrange(pkg, ctx):
    """group -> uint8 [columns, 2^k, 32] on the device, in Lagrange form: what the stages wrote, the byte columns as cells, blinded"""
    import torch
    rng = np.random.default_rng(0x6172726f7773)
    key, pts = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (BLOCKS, 16), dtype=np.uint8)
    d_key, d_pt = torch.from_numpy(key).cuda(), torch.from_numpy(pts).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    advice = ctx.assemble_advice(K, N_SETS, w, kw, BLOCKS, layout=PACKED)
    advice_fr = ctx.assemble_advice(K, N_SETS, w, kw, BLOCKS, layout=PACKED, as_fr=True)
    mult, rep = ctx.lookup_multiplicities(K, N_SETS, w, kw, [BLOCKS], PACKED)
    assert rep["misses"] == 0
    a, s, _prep = ctx.permuted_columns(K, N_SETS, mult, n_rows=U, pad_row=0)
    inputs, _irep = ctx.lookup_inputs(K, N_SETS, w, kw)
    table_fr, _trep = ctx.compress_table(THETA)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    a_fr = ctx.argument_columns(a, table_fr, K, N_SETS, n_rows=U, out=zeros(N_SETS, 5, N, 32)).reshape(-1, N, 32)
    s_fr = ctx.argument_columns(s, table_fr, K, N_SETS, n_rows=U, out=zeros(N_SETS, 5, N, 32)).reshape(-1, N, 32)
    inv, _vrep = ctx.invert_table(table_fr, BETA, GAMMA)
    z, _closing, grep_ = ctx.grand_product(K, N_SETS, inputs, a, s, table_fr, inv, BETA, GAMMA, n_rows=U, _out=(zeros(N_SETS, 5, N, 32), zeros(N_SETS, 5, 32)))
    assert grep_ == {"arguments": 5 * N_SETS, "open": 0, "first_open": None}
    sel, fixed = pkg.assemble_selectors(K, N_SETS, BLOCKS)
    mapping = pkg.api.permutation_mapping(K, N_SETS, BLOCKS)
    n_cols, n_perm = pkg.api.permutation_columns(N_SETS), qm.perm_sets(N_SETS, CHUNK_LEN)
    sigma_tables = ctx.permutation_tables(K, n_cols)
    d_fixed = torch.from_numpy(np.asarray(fixed, np.uint8).reshape(1, -1)).cuda()
    zp, _zc, srep = ctx.permutation_product(K, n_cols, CHUNK_LEN, advice, d_fixed, pkg.api.permutation_sources(N_SETS), mapping, sigma_tables, BETA, GAMMA,
                                            n_rows=U, _out=(zeros(n_perm, N, 32), zeros(n_perm, 32)))
    assert not srep["open"] and srep["zero_terms"] == 0
    sigma = ctx.permutation_columns_fr(K, n_cols, mapping, sigma_tables)

    def cells_of_bytes(columns):
        b = torch.from_numpy(np.ascontiguousarray(columns, np.uint8)).cuda()
        return ctx.expand_fr(b.reshape(-1)).reshape(b.shape[0], N, 32)
    sel = np.asarray(sel, np.uint8)
    table = np.zeros((4, N), np.uint8)
    table[:, :U] = ctx.lookup_table().cpu().numpy()[:, tm.table_column(U, 0)]
    groups = {"advice": advice_fr, "rcon": cells_of_bytes(np.stack([np.asarray(fixed, np.uint8).reshape(-1), sel[-1]])), "selectors": cells_of_bytes(sel[:5 * N_SETS]),
              "table": blind(cells_of_bytes(table), U, ar.BLIND_SEEDS["table"]), "sigma": sigma, "zperm": blind(zp, U + 1, ar.BLIND_SEEDS["zperm"]),
              "a": blind(a_fr, U, ar.BLIND_SEEDS["a"]), "s": blind(s_fr, U, ar.BLIND_SEEDS["s"]),
              "zlookup": blind(z.reshape(-1, N, 32), U + 1, ar.BLIND_SEEDS["zlookup"]), "l": cells_of_bytes(np.asarray(qm.unit_columns(K, U), np.uint8))}
    torch.cuda.synchronize()
    assert {g: t.shape[0] for g, t in groups.items()} == qm.group_columns(N_SETS, CHUNK_LEN)
    # a copied advice cell of set 0's x column inside the first block: sigma moves it
    first = pkg.api.block_placement(K, N_SETS, 0)[1]
    row = next(i for i in range(first + 2, first + 1300) if int(mapping[0][i]) != i)
    return groups, row


def prove(pkg, ctx, groups):
    """(lhs, rhs, h(x), the pieces' sum at x, the top coefficients of h) for the Lagrange groups: the pipeline and the identity at X"""
    import torch
    api = pkg.api
    tables = ctx.ntt_tables(EXT_K)
    points = torch.from_numpy(api.rotated_points(X, K, ROTATIONS)).cuda()
    coeff = {g: ctx.lagrange_to_coeff(t, K, tables) for g, t in groups.items()}
    extended = {g: ctx.coeff_to_extended(c, K, EXT_K, tables, ZETA_SEL) for g, c in coeff.items()}
    h_ext = ctx.quotient_extended(extended, K, EXT_K, ZETA_SEL, N_SETS, CHUNK_LEN, U, THETA, BETA, GAMMA, Y)
    h_coeff = ctx.extended_to_coeff(h_ext, EXT_K, tables, ZETA_SEL)
    at_x = {g: [nm.from_cells(col) for col in ctx.evaluate_columns(c, K, points).cpu().numpy()] for g, c in coeff.items()}
    at = lambda g, c, r: at_x[g][c][ROTATIONS.index(r)]  # noqa: E731
    lhs = qm.fold(qm.constraints(K, K, N_SETS, CHUNK_LEN, U, X, at, THETA, BETA, GAMMA), Y)
    h_x = nm.from_cells(ctx.evaluate_columns(h_coeff, EXT_K, [X]).cpu().numpy())[0]
    pieces = api.quotient_pieces(h_coeff, K, EXT_K)
    assert len(pieces) == 1 << (EXT_K - K) and all(p.shape == (N, 32) and p.data_ptr() == h_coeff.data_ptr() + 32 * N * i for i, p in enumerate(pieces))
    piece_x = nm.from_cells(ctx.evaluate_columns(torch.stack(pieces), K, [X]).cpu().numpy())
    summed = sum(pow(X, N * i, R) * v for i, v in enumerate(piece_x)) % R
    return lhs, h_x * (pow(X, N, R) - 1) % R, h_x, summed, nm.from_cells(h_coeff[-N:].cpu().numpy())


def test_the_identity_holds_on_a_real_circuit_fails_after_a_flipped_byte_and_the_pieces_sum_to_h(pkg, ctx, lagrange):
    groups, row = lagrange
    assert all(pow(X, 1 << EXT_K, R) != v for v in (1, pow(nm.ZETAS[ZETA_SEL], 1 << EXT_K, R)))  # x lies neither on the domain nor on the coset
    lhs, rhs, h_x, summed, top = prove(pkg, ctx, groups)
    assert lhs == rhs and lhs != 0 and h_x != 0
    assert summed == h_x
    # the numerator's degree is at most (chunk_len + 2)(n - 1), so h's is below 4 n - 4: its top coefficients are 0 and the last piece is short
    assert top[-4:] == [0, 0, 0, 0] and any(top)
    flipped = dict(groups, advice=groups["advice"].clone())
    flipped["advice"][0, row, 0] ^= 0x10
    lhs2, rhs2, _h, summed2, top2 = prove(pkg, ctx, flipped)
    assert lhs2 != rhs2 and lhs2 != lhs  # the numerator no longer vanishes on the domain: what the division gives is no quotient
    assert summed2 == _h                 # the pieces are still the coefficients' views
    assert top2[-4:] != [0, 0, 0, 0]     # ... and the degree bound is gone with the divisibility
