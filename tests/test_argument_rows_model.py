"""The quotient's rules on a real circuit, on the CPU: tests/quot_model.py's constraints over the columns the oracle and the five
stage models make -- oracle.circuit for advice, selectors, the fixed column and the copies; mult_model, perm_model, theta_model,
grand_model and sigma_model for the rest (argument_rows.model_groups) -- must all be 0 on the rows of argument_rows.rows_to_check,
the blinded rows among them.  This holds quot_model against the other models on data on which the constraints vanish; a rule that
compresses, rotates, numbers its columns or places l_last otherwise than the stages fails here.

Two shapes at k = 17, the smallest k that holds the table.  (17, 2, 150, 3), sigma_cases.CHAIN: permutation sets (0,3) (3,6)
(6,8), in full.  (17, 1, 95, 2): sets (0,2) (2,4) (4,5) and one column set filled to its capacity; grand_model's product over
2^17 rows is some 3 s an argument, so this shape leaves the lookup Z out and holds the gate, the permutation and A' against S'
(argument_rows.without_lookup_z) -- its lookup products run on the device in tests/test_gpu_argument_rows.py.
No case runs beta = 0: the all-zero table row compresses to 0, so A' + beta is 0 on every row whose selector is off, the models'
inv(0) = 0 zeroes Z from there on, and the product constraint then fails by the models' own convention, not by a rule."""
import numpy as np
import pytest

import argument_rows as ar
import sigma_cases as sc

K = 17
U = (1 << K) - 6
THETA, BETA, GAMMA = (sc.seeded(s) for s in (0x61727468, 0x61726265, 0x61726761))
EXTRA = 200
SHAPES = (sc.CHAIN, (17, 1, 95, 2))


def inputs(n_blocks):
    rng = np.random.default_rng(0x6172726f7773)
    return rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n_blocks, 16), dtype=np.uint8)


def test_the_names_number_the_constraints():
    for n_sets, chunk_len, count in ((2, 3, 58), (1, 2, 3 + 2 + 3 + 25), (4, 3, 3 + 4 + 5 + 100)):
        names = ar.CONSTRAINT_NAMES(n_sets, chunk_len)
        assert len(names) == len(set(names)) == count
    names = ar.CONSTRAINT_NAMES(2, 3)
    assert names[:8] == ["gate", "perm.l0", "perm.last", "perm.chain[1]", "perm.chain[2]", "perm.product[0]", "perm.product[1]", "perm.product[2]"]
    assert names[8:13] == ["lookup[0,1].l0", "lookup[0,1].last", "lookup[0,1].product", "lookup[0,1].first", "lookup[0,1].adjacent"] and names[-1] == "lookup[1,5].adjacent"


def test_the_row_set_holds_its_fixed_part(oracle):
    k, n_sets, n_blocks, _ = sc.CHAIN
    with oracle.circuit(k, n_sets, *inputs(n_blocks), record_copies=False) as c:
        firsts = ar.blocks_of_sets(c, k, n_sets, n_blocks)
        rows = ar.rows_to_check(c, k, n_sets, n_blocks, U, 7, EXTRA)
        fixed = ar.rows_to_check(c, k, n_sets, n_blocks, U, 7, 0)
    assert rows == sorted(set(rows)) and set(fixed) <= set(rows) and len(fixed) < len(rows) <= len(fixed) + EXTRA
    have = set(fixed)
    assert {0, 1, (1 << k) - 1} <= have and set(range(496)) <= have and set(range(66550, 66571)) <= have and set(range(U - 2, 1 << k)) <= have
    assert [len(f) > 1 for f in firsts] == [True, True]
    for f in firsts:
        assert set(range(f[0], f[0] + 1360)) <= have and set(range(f[-1], f[-1] + 1360 + ar.BEHIND)) <= have and f[-1] + 1360 + ar.BEHIND <= U
    assert 3500 < len(fixed) < 5000


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "k%d-n%d-b%d-l%d" % s)
def test_every_constraint_is_zero_on_the_models_columns(oracle, shape):
    k, n_sets, n_blocks, chunk_len = shape
    full = shape == sc.CHAIN
    key, pts = inputs(n_blocks)
    with oracle.circuit(k, n_sets, key, pts, record_copies=False) as c:
        rows = ar.rows_to_check(c, k, n_sets, n_blocks, U, 0x726f77, EXTRA)
        last = c.block_placement(n_blocks - 1)
        assert last[1] + ar.AES_ROWS <= U
    if not full:  # the largest circuit of one set: its capacity (95 blocks) binds before the usable rows do, and a block more is refused
        assert n_sets == 1
        with oracle.circuit(k, n_sets, key, np.concatenate([pts, pts[:1]]), record_copies=False) as c:
            assert c.status != 0
    groups, facts = ar.model_groups(oracle, k, n_sets, chunk_len, key, pts, THETA, BETA, GAMMA, rows, lookup_z=full)
    assert facts["perm_report"] == {"sets": 3, "open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}
    if full:
        assert facts["grand_report"] == {"arguments": 5 * n_sets, "open": 0, "first_open": None}
    found = ar.violations(groups, rows, k, n_sets, chunk_len, U, THETA, BETA, GAMMA, only=None if full else ar.without_lookup_z)
    assert not found, "%d violations, the first %r" % (len(found), sorted(ar.named(found, n_sets, chunk_len))[:12])
    # Row U - 1 is idle in every column of a circuit this configuration can place (no copy, no lookup: every Z[U - 1] = Z[U]), so a
    # rule with l_last or the chain's rotation at U - 1 vanishes on these columns too.  A changed closing cell tells U from U - 1.
    ends = [0, 1, U - 2, U - 1, U, U + 1]
    closing = [("zperm", 0, {(0, "perm.chain[1]"), (U - 1, "perm.product[0]")}), ("zperm", 2, {(U, "perm.last"), (U - 1, "perm.product[2]")})]
    if full:
        closing.append(("zlookup", 7, {(U, "lookup[1,3].last"), (U - 1, "lookup[1,3].product")}))
    for g, c, expected in closing:
        groups[g][c][U] += 1
        got = ar.named(ar.violations(groups, ends, k, n_sets, chunk_len, U, THETA, BETA, GAMMA, only=None if full else ar.without_lookup_z), n_sets, chunk_len)
        groups[g][c][U] -= 1
        assert got == expected, (g, c)
    # the columns are no trivial ones: another theta or beta is noticed, where the rule says it is
    other = ar.named(ar.violations(groups, rows[:600], k, n_sets, chunk_len, U, THETA + 1, BETA, GAMMA, only=None if full else ar.without_lookup_z), n_sets, chunk_len)
    assert {name for _i, name in other} == ({"lookup[%d,%d].product" % (s, t) for s in range(n_sets) for t in range(1, 6)} if full else set())
    other = ar.named(ar.violations(groups, rows[:600], k, n_sets, chunk_len, U, THETA, BETA + 1, GAMMA, only=ar.without_lookup_z), n_sets, chunk_len)
    # ... in every set that holds a copied column: the fixed column (4) is copied nowhere, and where it is a set alone, Z is constant
    copied = [s for s, (first, end) in enumerate(ar.sm.sets_of(ar.sm.columns(n_sets), chunk_len)) if set(range(first, end)) != {4}]
    assert copied == ([0, 1, 2] if full else [0, 1]) and {name for _i, name in other} == {"perm.product[%d]" % s for s in copied}
