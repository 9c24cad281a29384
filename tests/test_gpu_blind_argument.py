"""A prover's blinding must not disturb the argument: the device chain of tests/test_gpu_argument_rows.py at its smaller shape,
(17, 1, 95, 2), with every group that argument_rows.blind_groups blinds on the host -- both Z above n_rows, A', S' and the raw table
columns from n_rows -- blinded on the device instead, by Context.blind_rows under one seed and one domain a group, at
argument_rows.FIRST_BLIND's offsets.  Then every named constraint of tests/quot_model.py is zero on argument_rows.rows_to_check,
which holds the rows n_rows ... 2^k - 1 and row 0, whose rotation -1 reads a blinding cell; every cell above n_rows is
tests/blind_model.py's (all of them: 22 columns of five or six rows, no sample needed); and no row a stage wrote has changed."""
import numpy as np
import pytest

import argument_rows as ar
import blind_cases as bc
import blind_model as bm
import guarded as G
import sigma_cases as sc

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, BLOCKS, CHUNK_LEN = SHAPE = (17, 1, 95, 2)
N_ROWS = 1 << K
U = N_ROWS - 6
THETA, BETA, GAMMA = (sc.seeded(s) for s in (0x61727468, 0x61726265, 0x61726761))  # tests/test_gpu_argument_rows.py's
EXTRA = 200
POISON = 0xA5
DOMAINS = {g: 1 + i for i, g in enumerate(sorted(ar.BLIND_SEEDS))}  # one domain a group, under the one seed


def on_rows(t, rows):
    import torch
    return t[:, torch.as_tensor(rows, device=t.device)].cpu().numpy()


@pytest.fixture(scope="module")
def world(pkg, ctx, oracle):
    import torch
    k, n_sets, n, chunk_len = SHAPE
    rng = np.random.default_rng(0x6172726f7773)
    key, pts = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
    d_key, d_pt = torch.from_numpy(key).cuda(), torch.from_numpy(pts).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    advice = ctx.assemble_advice(k, n_sets, w, kw, n, layout=PACKED)
    advice_fr = ctx.assemble_advice(k, n_sets, w, kw, n, layout=PACKED, as_fr=True)
    mult, rep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n], PACKED)
    assert rep["misses"] == 0
    a, s, prep = ctx.permuted_columns(k, n_sets, mult, n_rows=U, pad_row=0)
    assert prep["overflowed"] == 0
    inputs, _irep = ctx.lookup_inputs(k, n_sets, w, kw)
    table_fr, _trep = ctx.compress_table(THETA)
    poisoned = lambda *shape: torch.full(shape, POISON, dtype=torch.uint8, device="cuda")  # noqa: E731
    a_fr = ctx.argument_columns(a, table_fr, k, n_sets, n_rows=U, out=poisoned(n_sets, 5, N_ROWS, 32))
    s_fr = ctx.argument_columns(s, table_fr, k, n_sets, n_rows=U, out=poisoned(n_sets, 5, N_ROWS, 32))
    inv, _vrep = ctx.invert_table(table_fr, BETA, GAMMA)
    z, _closing, grep_ = ctx.grand_product(k, n_sets, inputs, a, s, table_fr, inv, BETA, GAMMA, n_rows=U, _out=(poisoned(n_sets, 5, N_ROWS, 32), poisoned(n_sets, 5, 32)))
    assert grep_["open"] == 0
    sel, fixed = pkg.assemble_selectors(k, n_sets, n)
    mapping = pkg.api.permutation_mapping(k, n_sets, n)
    n_cols = pkg.api.permutation_columns(n_sets)
    n_perm = pkg.api.permutation_sets(n_sets, chunk_len)
    tables = ctx.permutation_tables(k, n_cols)
    d_fixed = torch.from_numpy(np.asarray(fixed, np.uint8).reshape(1, -1)).cuda()
    zp, _zp_closing, srep = ctx.permutation_product(k, n_cols, chunk_len, advice, d_fixed, pkg.api.permutation_sources(n_sets), mapping, tables, BETA, GAMMA,
                                                    n_rows=U, _out=(poisoned(n_perm, N_ROWS, 32), poisoned(n_perm, 32)))
    assert not srep["open"]
    sigma = ctx.permutation_columns_fr(k, n_cols, mapping, tables)
    # the raw table columns have no device column of their own in the chain: their blinding rows are filled into a poisoned one
    device = {"table": poisoned(4, N_ROWS, 32), "zperm": zp, "a": a_fr.reshape(-1, N_ROWS, 32), "s": s_fr.reshape(-1, N_ROWS, 32), "zlookup": z.reshape(-1, N_ROWS, 32)}
    assert set(device) == set(ar.BLIND_SEEDS) == set(ar.FIRST_BLIND)
    torch.cuda.synchronize()
    before = {g: t.clone() for g, t in device.items()}
    # ---- the prover's blinding, on the device: what argument_rows.blind_groups does on the host
    seed = ctx.blinding_seed(bc.SEED)
    for g, t in device.items():
        assert ctx.blind_rows(t, k, U + ar.FIRST_BLIND[g], seed, DOMAINS[g]) is t
    torch.cuda.synchronize()

    rows = ar.rows_to_check(pkg, k, n_sets, n, U, 0x726f77, EXTRA)
    need = ar.read_rows(rows, k, U)
    decode = lambda t: ar.cell_columns(on_rows(t, need), k, need)  # noqa: E731
    table = ar.table_group(ctx.lookup_table().cpu().numpy(), k, U, 0)
    tail = ar.cell_columns(device["table"][:, U:].cpu().numpy(), k, range(U, N_ROWS))
    for column, blinded in zip(table, tail):
        assert all(v is None for v in column[U:])
        column[U:] = blinded[U:]
    groups = {"advice": decode(advice_fr), "rcon": ar.rcon_group(sel, fixed), "selectors": ar.selectors_group(sel, n_sets), "table": table, "sigma": decode(sigma),
              "zperm": decode(device["zperm"]), "a": decode(device["a"]), "s": decode(device["s"]), "zlookup": decode(device["zlookup"]), "l": ar.unit_columns(k, U)}
    return dict(groups=groups, rows=rows, need=need, device=device, before=before)


def test_every_constraint_is_zero_on_the_columns_the_device_blinded(world):
    k, n_sets, _n, chunk_len = SHAPE
    rows = world["rows"]
    assert set(range(U, N_ROWS)) <= set(rows) and 0 in rows  # the blinded rows themselves, and the row whose rotation -1 reads one
    bad = ar.named(ar.violations(world["groups"], rows, k, n_sets, chunk_len, U, THETA, BETA, GAMMA), n_sets, chunk_len)
    assert not bad, "%d violations, the first %r" % (len(bad), sorted(bad)[:12])


def test_the_cells_above_n_rows_are_the_models_and_no_other_row_changed(world):
    import torch
    seen = set()
    for g, t in world["device"].items():
        first = U + ar.FIRST_BLIND[g]
        G.assert_bytes("the blinding rows of %s" % g, t[:, first:].cpu().numpy(), bm.tail_cells(bc.SEED, K, t.shape[0], first, DOMAINS[g]))
        assert torch.equal(t[:, :first], world["before"][g][:, :first]), g  # what the stages wrote, and the poison below the table's tail
        assert bool((world["before"][g][:, first:] == POISON).all()), g    # the rows blinded are the rows no stage wrote
        cells = {r.tobytes() for r in t[:, first:].cpu().numpy().reshape(-1, 32)}
        assert len(cells) == t.shape[0] * (N_ROWS - first) and not cells & seen, g  # no cell twice, within a group or across the groups
        seen |= cells
