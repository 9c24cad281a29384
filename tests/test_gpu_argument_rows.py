"""The device's columns held to the circuit's own constraints: one key, one set of plaintexts and one theta, beta, gamma through
every prover stage on the GPU -- the witness, the advice as bytes and as cells, the multiplicities, A' and S', the input column,
the compressed tables, the inverse table, the lookup Z, the mapping, the permutation Z and sigma as cells -- and then
tests/quot_model.py's constraints (argument_rows.violations) over the finished columns: every one of them 0 on the rows of
argument_rows.rows_to_check, for (17, 2, 150, 3) and for (17, 1, 95, 2), a column set filled to its capacity.  The rows no stage
writes (both Z above n_rows, A' and S' from n_rows; poisoned outputs say which) and the raw table columns' tail are blinded with
seeded random cells first, so the constraints have to vanish on rows n_rows ... 2^k - 1 as well and row 0's rotation -1 reads
a random cell.

The corruptions change one cell of the finished columns, put it back afterwards and recompute nothing; no kernel is mutated.
Each expected set of (row, constraint) is derived from the rule in the comment beside it and must be met exactly.
The model chain of tests/test_argument_rows_model.py gives the same columns cell for cell; grand_model's product is left out of
that comparison (tests/test_gpu_grand_chain.py holds every cell of the lookup Z of this shape against it already, and it alone
would take longer than the rest of this file).  No graph capture here: the stages' own tests hold it."""
import contextlib

import numpy as np
import pytest

import argument_rows as ar
import ntt_model as nm
import quot_model as qm
import sigma_cases as sc
import sigma_model as sm

pytestmark = pytest.mark.gpu
PACKED = 1
K = 17
N_ROWS = 1 << K
U = N_ROWS - 6
THETA, BETA, GAMMA = (sc.seeded(s) for s in (0x61727468, 0x61726265, 0x61726761))  # tests/test_argument_rows_model.py's
EXTRA = 200
POISON = 0xA5
SHAPES = (sc.CHAIN, (17, 1, 95, 2))
BINS = 66561


def on_rows(t, rows):
    import torch
    return t[:, torch.as_tensor(rows, device=t.device)].cpu().numpy()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "k%d-n%d-b%d-l%d" % s)
def world(request, pkg, ctx, oracle):
    import torch
    k, n_sets, n, chunk_len = request.param
    assert k == K and n <= pkg.block_capacity(k, n_sets) and pkg.api.block_placement(k, n_sets, n - 1)[1] + pkg.AES_ROWS <= U
    if n_sets == 1:
        assert n == pkg.block_capacity(k, n_sets)  # the set is full: 95 blocks, the capacity binds before the usable rows do
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
    inputs, irep = ctx.lookup_inputs(k, n_sets, w, kw)
    assert irep == rep
    table_fr, trep = ctx.compress_table(THETA)
    assert not trep["noncanonical"]
    poisoned = lambda *shape: torch.full(shape, POISON, dtype=torch.uint8, device="cuda")
    a_fr = ctx.argument_columns(a, table_fr, k, n_sets, n_rows=U, out=poisoned(n_sets, 5, N_ROWS, 32))
    s_fr = ctx.argument_columns(s, table_fr, k, n_sets, n_rows=U, out=poisoned(n_sets, 5, N_ROWS, 32))
    inv, vrep = ctx.invert_table(table_fr, BETA, GAMMA)
    assert vrep == {"cells": 2 * 3 * BINS, "noncanonical": False, "zero_terms": 0}
    z, closing, grep_ = ctx.grand_product(k, n_sets, inputs, a, s, table_fr, inv, BETA, GAMMA, n_rows=U,
                                          _out=(poisoned(n_sets, 5, N_ROWS, 32), poisoned(n_sets, 5, 32)))
    assert grep_ == {"arguments": 5 * n_sets, "open": 0, "first_open": None}
    sel, fixed = pkg.assemble_selectors(k, n_sets, n)
    assert np.array_equal(fixed[:96], pkg.selector_tags()[3]) and not fixed[96:].any()
    mapping = pkg.api.permutation_mapping(k, n_sets, n)
    n_cols = pkg.api.permutation_columns(n_sets)
    n_perm = qm.perm_sets(n_sets, chunk_len)
    assert n_cols == sm.columns(n_sets) and n_perm == 3
    tables = ctx.permutation_tables(k, n_cols)
    d_fixed = torch.from_numpy(np.asarray(fixed, np.uint8).reshape(1, -1)).cuda()
    zp, zp_closing, srep = ctx.permutation_product(k, n_cols, chunk_len, advice, d_fixed, pkg.api.permutation_sources(n_sets), mapping, tables, BETA, GAMMA,
                                                   n_rows=U, _out=(poisoned(n_perm, N_ROWS, 32), poisoned(n_perm, 32)))
    assert srep == {"sets": n_perm, "open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}
    sigma = ctx.permutation_columns_fr(k, n_cols, mapping, tables)
    torch.cuda.synchronize()
    # the rows a prover blinds are the rows the device left alone, and no other
    for t, first in ((z.reshape(-1, N_ROWS, 32), U + 1), (zp, U + 1), (a_fr.reshape(-1, N_ROWS, 32), U), (s_fr.reshape(-1, N_ROWS, 32), U)):
        assert bool((t[:, first:] == POISON).all()) and not bool((t[:, :first] == POISON).all(dim=2).any())
    assert bytes(closing.cpu().numpy().reshape(-1, 32)[-1]) == sm.ONE_CELL and bytes(zp_closing[-1].cpu().numpy()) == sm.ONE_CELL

    rows = ar.rows_to_check(pkg, k, n_sets, n, U, 0x726f77, EXTRA)
    need = ar.read_rows(rows, k, U)
    written = lambda first: [i for i in need if i < first]
    adv_bytes = advice.cpu().numpy()
    groups = {"advice": ar.cell_columns(on_rows(advice_fr, need), k, need), "rcon": ar.rcon_group(sel, fixed), "selectors": ar.selectors_group(sel, n_sets),
              "table": ar.table_group(ctx.lookup_table().cpu().numpy(), k, U, 0), "sigma": ar.cell_columns(on_rows(sigma, need), k, need),
              "zperm": ar.cell_columns(on_rows(zp, written(U + 1)), k, written(U + 1)),
              "a": ar.cell_columns(on_rows(a_fr.reshape(-1, N_ROWS, 32), written(U)), k, written(U)),
              "s": ar.cell_columns(on_rows(s_fr.reshape(-1, N_ROWS, 32), written(U)), k, written(U)),
              "zlookup": ar.cell_columns(on_rows(z.reshape(-1, N_ROWS, 32), written(U + 1)), k, written(U + 1)), "l": ar.unit_columns(k, U)}
    assert all(groups["advice"][c][i] == int(adv_bytes[c, i]) for c in range(3 * n_sets + 1) for i in need)  # the cells decode to the byte columns
    assert np.array_equal(np.asarray(groups["table"])[:, :BINS].astype(np.uint8), oracle.lookup_table())
    ar.blind_groups(groups, U)
    return dict(shape=request.param, key=key, pts=pts, groups=groups, rows=rows, have=set(rows), sel=sel, fixed=fixed, mapping=mapping,
                a=a.cpu().numpy().reshape(-1, N_ROWS), s=s.cpu().numpy().reshape(-1, N_ROWS), first=pkg.api.block_placement(k, n_sets, 0)[1],
                behind=pkg.api.block_placement(k, n_sets, n - 1)[1] + pkg.AES_ROWS + 2)


def found(w, rows, theta=THETA, beta=BETA, gamma=GAMMA):
    k, n_sets, _n, chunk_len = w["shape"]
    assert set(rows) <= w["have"]  # rows whose rotations were decoded
    return ar.named(ar.violations(w["groups"], rows, k, n_sets, chunk_len, U, theta, beta, gamma), n_sets, chunk_len)


def test_every_constraint_is_zero_on_the_devices_columns(world):
    bad = found(world, world["rows"])
    assert not bad, "%d violations, the first %r" % (len(bad), sorted(bad)[:12])


# ---- corruptions -----------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def changed(w, group, column, row, value=None):
    col = w["groups"][group][column]
    old = col[row]
    assert old is not None
    col[row] = nm.seeded_values(1, 0x636f72 + row)[0] if value is None else value
    assert col[row] != old
    try:
        yield
    finally:
        col[row] = old


def around(*rows):
    return sorted({(i + d) % N_ROWS for i in rows for d in (-2, -1, 0, 1, 2)})


def inside(w):
    """the checked rows whose neighbourhood around() is checked too, away from both ends of the usable rows"""
    return [i for i in w["rows"] if 2 <= i < U - 3 and {i - 2, i - 1, i + 1, i + 2} <= w["have"]]


def advice_rule(w, column, row):
    """What the rule says of a changed advice cell: the lookup product of every tag of the cell's set whose selector is on at that
    row and whose arity reaches the cell's column (x: every tag, y: arity 3 and 4, z: the xor alone); the gate for the words
    column where q_rcon is on; and the product of the cell's permutation set exactly if sigma moves the cell -- where sigma is
    the cell's own label both sides of Z[i + 1] * prod(v + beta sigma + gamma) = Z[i] * prod(v + beta delta^c x + gamma) take
    the same new factor."""
    k, n_sets, _n, chunk_len = w["shape"]
    out = set()
    if column == 3 * n_sets:
        if w["sel"][5 * n_sets][row]:
            out.add((row, "gate"))
    else:
        st, operand = divmod(column, 3)
        out |= {(row, "lookup[%d,%d].product" % (st, t)) for t in range(1, 6) if w["sel"][5 * st + t - 1][row] and qm.ARITY[t] > operand + 1}
    c = sm.column_of_advice(n_sets, column)
    if int(w["mapping"][c][row]) != (c << k) + row:
        out.add((row, "perm.product[%d]" % (c // chunk_len)))
    return out


def test_a_changed_advice_cell_breaks_its_lookups_and_its_copies_and_a_free_cell_nothing(world):
    w = world
    k, n_sets, _n, chunk_len = w["shape"]
    block = range(w["first"] + 2, w["first"] + 1300)
    identity = lambda column, row: int(w["mapping"][sm.column_of_advice(n_sets, column)][row]) == (sm.column_of_advice(n_sets, column) << k) + row
    # x, y and z of the first checked row of every selector of set 0 (the range check's are key rows): the product of that tag exactly
    # if its arity reaches the column
    for i_sel in range(5):
        row = next(i for i in inside(w) if w["sel"][i_sel][i])
        for operand in range(3):
            expected = advice_rule(w, operand, row)
            assert ((row, "lookup[0,%d].product" % (i_sel + 1)) in expected) == (qm.ARITY[i_sel + 1] > operand + 1)
            with changed(w, "advice", operand, row, w["groups"]["advice"][operand][row] ^ 0x10):
                assert found(w, around(row)) == expected, (i_sel, operand)
    # a copy destination of every column of set 0, and of the words column: the permutation set of the column
    for column in (0, 1, 2, 3 * n_sets):
        rows = range(2, 90) if column == 3 * n_sets else block
        row = next(i for i in rows if not identity(column, i))
        expected = advice_rule(w, column, row)
        assert (row, "perm.product[%d]" % (sm.column_of_advice(n_sets, column) // chunk_len)) in expected
        with changed(w, "advice", column, row, w["groups"]["advice"][column][row] ^ 0x10):
            assert found(w, around(row)) == expected, column
    # z of the last set, two rows behind its last block: no selector, no copy, no constraint
    column, row = 3 * n_sets - 1, w["behind"]
    assert row + 2 < U and not w["sel"][5 * (n_sets - 1):5 * n_sets, row].any() and identity(column, row) and advice_rule(w, column, row) == set()
    with changed(w, "advice", column, row, 0x5a):
        assert found(w, around(row)) == set()


def test_a_changed_cell_of_a_permuted_column_breaks_the_product_and_its_neighbours(world):
    w = world
    a, s = w["a"], w["s"]
    rows = inside(w)
    for arg in sorted({1, 5 * (w["shape"][1] - 1) + 1}):  # the xor of the first and of the last set
        name = "lookup[%d,%d]." % (arg // 5, arg % 5 + 1)
        # A'[i] in front of a repeat (A'[i + 1] = A'[i] != S'[i + 1]): the product at i; adjacent at i -- the new cell is neither
        # S'[i] nor A'[i - 1] --; adjacent at i + 1, whose A'[i + 1] is neither S'[i + 1] nor the new A'[i]
        row = next(i for i in rows if a[arg][i + 1] == a[arg][i] != s[arg][i + 1])
        with changed(w, "a", arg, row):
            assert found(w, around(row)) == {(row, name + "product"), (row, name + "adjacent"), (row + 1, name + "adjacent")}
        # A'[i] in front of a new run (A'[i + 1] = S'[i + 1]): row i + 1 holds by its first factor
        row = next(i for i in rows if a[arg][i + 1] == s[arg][i + 1])
        with changed(w, "a", arg, row):
            assert found(w, around(row)) == {(row, name + "product"), (row, name + "adjacent")}
        # S'[i] where a run starts (A'[i] = S'[i] != A'[i - 1]): the product, and adjacent at i loses both factors
        row = next(i for i in rows if a[arg][i] == s[arg][i] and a[arg][i] != a[arg][i - 1])
        with changed(w, "s", arg, row):
            assert found(w, around(row)) == {(row, name + "product"), (row, name + "adjacent")}
        # S'[i] inside a run (A'[i] = A'[i - 1]): adjacent holds by its second factor
        row = next(i for i in rows if a[arg][i] == a[arg][i - 1])
        with changed(w, "s", arg, row):
            assert found(w, around(row)) == {(row, name + "product")}


def test_a_changed_cell_of_a_lookup_z_breaks_the_rows_that_read_it(world):
    w = world
    arg = 5 * (w["shape"][1] - 1) + 2  # the S-box of the last set
    name = "lookup[%d,3]." % (arg // 5)
    row = w["first"] + 700
    with changed(w, "zlookup", arg, row):  # Z[i] is the right side's at i and the left side's at i - 1
        assert found(w, around(row)) == {(row - 1, name + "product"), (row, name + "product")}
    with changed(w, "zlookup", arg, 0):  # l0 * (1 - Z); the row in front, 2^k - 1, is not active
        assert found(w, around(0)) == {(0, name + "l0"), (0, name + "product")}
    with changed(w, "zlookup", arg, U):  # l_last * (Z^2 - Z); row U itself is not active
        assert found(w, around(U)) == {(U, name + "last"), (U - 1, name + "product")}


def test_a_changed_cell_of_a_permutation_z_breaks_the_chain_or_the_end(world):
    w = world
    with changed(w, "zperm", 0, U):  # Z_1[0] = Z_0[n_rows] is read at row 0; perm.last reads the last set alone
        assert found(w, around(0, U)) == {(0, "perm.chain[1]"), (U - 1, "perm.product[0]")}
    with changed(w, "zperm", 2, U):
        assert found(w, around(0, U)) == {(U, "perm.last"), (U - 1, "perm.product[2]")}
    with changed(w, "zperm", 1, 0):  # the chained cell itself: the chain that ends in it, and the product's right side at row 0
        assert found(w, around(0, U)) == {(0, "perm.chain[1]"), (0, "perm.product[1]")}
    with changed(w, "zperm", 0, 0):
        assert found(w, around(0, U)) == {(0, "perm.l0"), (0, "perm.product[0]")}


def test_a_changed_sigma_selector_round_constant_or_table_cell(world):
    w = world
    k, n_sets, _n, chunk_len = w["shape"]
    row = w["first"] + 333
    for c in range(sm.columns(n_sets)):  # a sigma cell is one factor of its set's left side
        with changed(w, "sigma", c, row):
            assert found(w, around(row)) == {(row, "perm.product[%d]" % (c // chunk_len))}, c
    # the S-box selector of the last set on in the free row behind its last block: the input is 3 theta^2 where A' holds a zero
    st, row = n_sets - 1, w["behind"]
    assert not w["sel"][5 * st:5 * st + 5, row].any() and w["groups"]["selectors"][5 * st + 2][row] == 0
    with changed(w, "selectors", 5 * st + 2, row, 1):
        assert found(w, around(row)) == {(row, "lookup[%d,3].product" % st)}
    # the round constant of a row with q_rcon on: the gate; the fixed column's sigma is the identity, so its product holds
    row = next(i for i in range(2, 96) if w["sel"][5 * n_sets][i])
    with changed(w, "rcon", 0, row, w["groups"]["rcon"][0][row] ^ 1):
        assert found(w, around(row)) == {(row, "gate")}
    # a raw table cell of column e is read by every argument of an arity above e, in the table and in the pad tail alike
    for row in (66555, 66565):
        for e in range(4):
            with changed(w, "table", e, row, w["groups"]["table"][e][row] + 1):
                assert found(w, around(row)) == {(row, "lookup[%d,%d].product" % (s_, t)) for s_ in range(n_sets) for t in range(1, 6) if qm.ARITY[t] > e}, (row, e)


def test_the_shared_challenges_matter(world):
    w = world
    n_sets = w["shape"][1]
    rows = w["rows"][:600]
    products = {"lookup[%d,%d].product" % (s_, t) for s_ in range(n_sets) for t in range(1, 6)}  # every arity is above 1
    # an argument no row looks up (the range check of a set without key rows) has A' = input = 0 on every row: beta multiplies both sides
    used = {"lookup[%d,%d].product" % (s_, t) for s_ in range(n_sets) for t in range(1, 6) if w["sel"][5 * s_ + t - 1].any()}
    assert len(products - used) == n_sets - 1
    assert {name for _i, name in found(w, rows, theta=sc.seeded(0x61727432))} == products
    assert {name for _i, name in found(w, rows, beta=sc.seeded(0x61726232))} == used | {"perm.product[0]", "perm.product[1]"} | \
        ({"perm.product[2]"} if n_sets > 1 else set())  # at one set the last permutation set is the fixed column alone: Z is constant
    assert {name for _i, name in found(w, rows, gamma=sc.seeded(0x61726732))} >= products


def test_the_devices_columns_are_the_model_chains(world, oracle):
    w = world
    k, n_sets, _n, chunk_len = w["shape"]
    rows = [int(i) for i in np.random.default_rng(0x6167726565).choice(w["rows"], 300, replace=False)]
    model, facts = ar.model_groups(oracle, k, n_sets, chunk_len, w["key"], w["pts"], THETA, BETA, GAMMA, rows, lookup_z=False)
    assert np.array_equal(facts["mapping"], w["mapping"]) and np.array_equal(facts["sel"], w["sel"]) and np.array_equal(facts["fixed"], w["fixed"])
    for g in qm.GROUPS:
        if g == "zlookup":  # tests/test_gpu_grand_chain.py's, in full
            continue
        for c, (mine, theirs) in enumerate(zip(model[g], w["groups"][g])):
            bad = [i for i in facts["need"] if mine[i] != theirs[i]]
            assert not bad, (g, c, bad[:5])
