"""A MockProver for the whole argument of a FixedAes128Config<k, n_sets> circuit -- the gate, the permutation argument and all
5 * n_sets lookups -- over finished Lagrange columns: tests/quot_model.py's constraints() at x = omega^row with a plain index
mod 2^k as the rotation, every constraint of which must be 0 on every row of the domain.  The columns are the caller's: the
stage models' (model_groups below, tests/test_argument_rows_model.py) or the device's (tests/test_gpu_argument_rows.py).  The
builders only turn bytes and 32-byte cells into Python integers, and cells are decoded by sigma_model.values.

A column is a list of 2^k entries.  One built from cells holds integers at the rows that were decoded and None elsewhere, so a
read the caller did not provide for ends in a TypeError, not in a zero."""
import numpy as np

import ntt_model as nm
import quot_model as qm
import sigma_model as sm
import theta_model as tm

R = qm.R
AES_ROWS, KEY_ROWS, WORDS_ROWS = 1360, 400, 96
BEHIND = 8  # rows checked behind the last block of a set


def perm_sets(n_sets, chunk_len):
    return qm.perm_sets(n_sets, chunk_len)


def CONSTRAINT_NAMES(n_sets, chunk_len):
    """A name for every index of quot_model.constraints' output, in its order."""
    sets = perm_sets(n_sets, chunk_len)
    names = ["gate", "perm.l0", "perm.last"]
    names += ["perm.chain[%d]" % s for s in range(1, sets)]
    names += ["perm.product[%d]" % s for s in range(sets)]
    for s in range(n_sets):
        for t in range(1, 6):
            names += ["lookup[%d,%d].%s" % (s, t, what) for what in ("l0", "last", "product", "first", "adjacent")]
    return names


def read_rows(rows, k, n_rows):
    """The sorted rows constraints() reads when it is asked for `rows`: rotations 0, 1, -1 and n_rows."""
    n = 1 << k
    return sorted({(i + r) % n for i in rows for r in (0, 1, -1, n_rows)})


def violations(groups, rows, k, n_sets, chunk_len, n_rows, theta, beta, gamma, only=None):
    """[(row, constraint index)] of every constraint that is not 0 at a row of `rows`; only(name): the constraints to look at
    (default: all)."""
    n, w = 1 << k, nm.omega(k)
    assert w == sm.omega(k) and set(groups) == set(qm.GROUPS)
    names = CONSTRAINT_NAMES(n_sets, chunk_len)
    look = [only is None or bool(only(name)) for name in names]
    out = []
    for i in rows:
        got = qm.constraints(k, k, n_sets, chunk_len, n_rows, pow(w, i, R), lambda g, c, r, i=i: groups[g][c][(i + r) % n], theta, beta, gamma)
        assert len(got) == len(names)
        out += [(i, j) for j, v in enumerate(got) if v and look[j]]
    return out


def without_lookup_z(name):
    """The constraints no lookup Z takes part in: the gate, the permutation's, and A' against S' of every lookup"""
    return not name.startswith("lookup") or name.endswith((".first", ".adjacent"))


def named(found, n_sets, chunk_len):
    """violations()' list as a set of (row, constraint name)"""
    names = CONSTRAINT_NAMES(n_sets, chunk_len)
    return {(i, names[j]) for i, j in found}


def blocks_of_sets(geometry, k, n_sets, n_blocks):
    """[set] -> the first rows of its blocks in order.  geometry: placement(b) -> (set, first row), or an object whose
    block_placement is that (the oracle's circuit), or the package (block_placement(k, n_sets, b))."""
    if callable(geometry):
        place = geometry
    elif hasattr(geometry, "api"):
        place = lambda b: geometry.api.block_placement(k, n_sets, b)
    else:
        place = geometry.block_placement
    firsts = [[] for _ in range(n_sets)]
    for b in range(n_blocks):
        s, first = place(b)
        firsts[s].append(first)
    return firsts


def rows_to_check(geometry, k, n_sets, n_blocks, n_rows, seed, extra):
    """The sorted rows the argument is held on: 0, 1 and 2^k - 1; the key rows 0 ... 495; every row of the first and of the last
    block of each set and the BEHIND rows behind the last; 66550 ... 66570, the end of the table; n_rows - 2 ... 2^k - 1; and
    `extra` seeded rows."""
    n = 1 << k
    rows = {0, 1, n - 1} | set(range(KEY_ROWS + WORDS_ROWS)) | set(range(66550, 66571)) | set(range(n_rows - 2, n))
    for firsts in blocks_of_sets(geometry, k, n_sets, n_blocks):
        if firsts:
            rows |= set(range(firsts[0], firsts[0] + AES_ROWS)) | set(range(firsts[-1], firsts[-1] + AES_ROWS + BEHIND))
    rows |= {int(i) for i in np.random.default_rng(seed).integers(0, n, extra)}
    assert all(0 <= i < n for i in rows)
    return sorted(rows)


# ---- builders ------------------------------------------------------------------------------------------------------------------------

def byte_columns(columns):
    """uint8 [count, 2^k] -> count lists of integers"""
    return [[int(v) for v in col] for col in np.asarray(columns).tolist()]


def cell_columns(cells, k, rows=None):
    """uint8 [count, len(rows), 32] canonical Montgomery cells of the rows `rows` (default: all 2^k, in order) -> count lists of
    2^k entries, None at every row that is not in `rows`."""
    cells = np.ascontiguousarray(cells, np.uint8)
    rows = list(range(1 << k)) if rows is None else list(rows)
    assert cells.ndim == 3 and cells.shape[1:] == (len(rows), 32)
    out = []
    for c in range(cells.shape[0]):
        col = [None] * (1 << k)
        for i, v in zip(rows, sm.values(cells[c])):
            col[i] = v
        out.append(col)
    return out


def unit_columns(k, n_rows):
    return qm.unit_columns(k, n_rows)


def table_group(table, k, n_rows, pad_row):
    """The four raw table columns over the usable rows: lookup_table() [4, 66561] read through theta_model.table_column; None from
    row n_rows on, the caller's to blind."""
    table = np.asarray(table)
    assert table.shape == (4, tm.BINS)
    index = tm.table_column(n_rows, pad_row)
    return [[int(v) for v in table[e][index].tolist()] + [None] * ((1 << k) - n_rows) for e in range(4)]


def rcon_group(selectors, fixed):
    """(the fixed round-constant column, its selector): assemble_selectors' / the oracle's last selector column and fixed column"""
    selectors = np.asarray(selectors)
    assert selectors.shape[0] % 5 == 1
    return byte_columns([np.asarray(fixed).reshape(-1), selectors[-1]])


def selectors_group(selectors, n_sets):
    """The 5 * n_sets lookup selectors in the rule's order 5 * s + tag - 1: assemble_selectors' rows (range, xor, sbox, mul2, mul3 of
    every set) are in it, mult_model.TAGS = theta_model.TAGS = 1 ... 5 in row order"""
    assert tm.TAGS == (1, 2, 3, 4, 5) and np.asarray(selectors).shape[0] == 5 * n_sets + 1
    return byte_columns(np.asarray(selectors)[:5 * n_sets])


def blind(columns, first, seed):
    """Fills rows first ... 2^k - 1 of every column with seeded canonical random values; every one of those rows must be None: a
    row nobody wrote."""
    for c, col in enumerate(columns):
        tail = len(col) - first
        assert all(v is None for v in col[first:]), "a row to blind holds a value"
        col[first:] = nm.seeded_values(tail, seed + c)
    return columns


# ---- the model chain -----------------------------------------------------------------------------------------------------------------

BLIND_SEEDS = {"table": 0x626c00, "zperm": 0x626c10, "a": 0x626c20, "s": 0x626c40, "zlookup": 0x626c60}
FIRST_BLIND = {"table": 0, "a": 0, "s": 0, "zperm": 1, "zlookup": 1}  # the first blinded row above n_rows: both Z hold their closing cell at n_rows


def blind_groups(groups, n_rows):
    """The rows a prover blinds and no stage writes: both Z above n_rows, A', S' and the raw table columns from n_rows."""
    for g, seed in BLIND_SEEDS.items():
        blind(groups[g], n_rows + FIRST_BLIND[g], seed)
    return groups


def model_groups(oracle, k, n_sets, chunk_len, key, pts, theta, beta, gamma, rows, pad_row=0, lookup_z=True):
    """(groups, facts): the ten column groups of the circuit oracle.circuit(k, n_sets, key, pts) from the oracle and the stage
    models alone -- mult_model, perm_model, theta_model, grand_model, sigma_model -- decoded at read_rows(rows), blinded, with
    n_rows = 2^k - 6.  lookup_z=False leaves grand_model's product out, by far the longest stage: the lookup Z are then columns
    of zeros, a stand-in that satisfies nothing, and the caller checks without_lookup_z alone.  facts: what the callers assert or
    reuse (the block placement, the mapping, the selectors, the advice bytes, the models' reports)."""
    import grand_model as gm
    import mult_model as mm
    import perm_model as pm
    n, u = 1 << k, (1 << k) - 6
    need = read_rows(rows, k, u)
    below = [i for i in need if i < u]
    with oracle.circuit(k, n_sets, key, pts) as c:
        assert c.status == 0 and c.num_rows == n and c.num_advice == 3 * n_sets + 1 and c.num_selectors == 5 * n_sets + 1
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
        fixed, copies = c.fixed(), c.copies().astype(np.int64)
        places = [c.block_placement(b) for b in range(len(pts))]
    column = [sm.column_of_advice(n_sets, a) for a in range(3 * n_sets + 1)]
    edges = [(column[dc] * n + dr, column[sc_] * n + sr) for sc_, sr, dc, dr in copies.tolist()]
    mapping = sm.mapping(k, n_sets, edges)
    buffers = np.concatenate([adv, fixed.reshape(1, -1)])
    perm_columns = [buffers[s] for s in sm.sources(n_sets)]
    z_perm, perm_report = sm.product_batched(k, perm_columns, mapping, beta, gamma, chunk_len, u)
    w, w_pows, acc = sm.omega(k), [], 1
    for _ in range(n):
        w_pows.append(acc)
        acc = acc * w % R
    d_pows = [pow(sm.DELTA, c_, R) for c_ in range(sm.columns(n_sets))]
    sigma = []
    for c_ in range(sm.columns(n_sets)):
        col = [None] * n
        for i in need:
            col[i] = sm.label(k, w_pows, d_pows, int(mapping[c_][i]))
        sigma.append(col)
    table = oracle.lookup_table()
    groups = {"advice": byte_columns(adv), "rcon": rcon_group(sel, fixed), "selectors": selectors_group(sel, n_sets), "table": table_group(table, k, u, pad_row),
              "sigma": sigma, "zperm": [col + [None] * (n - u - 1) for col in z_perm], "l": unit_columns(k, u)}
    facts = dict(adv=adv, sel=sel, fixed=fixed, mapping=mapping, places=places, perm_report=perm_report, need=need)
    tables_fr = tm.compressed_tables(table, theta)
    hist, misses = mm.multiplicities(adv, sel, oracle.tables())
    inputs, _lookups, input_misses = tm.input_columns(adv, sel, oracle.tables())
    assert misses == 0 and input_misses == 0
    a, s = np.zeros((n_sets, 5, u), np.int64), np.zeros((n_sets, 5, u), np.int64)
    for st in range(n_sets):
        for tag in pm.TAGS:
            a[st, tag - 1], s[st, tag - 1], over = pm.arrange(hist[st], tag, u, pad_row)
            assert not over
    facts.update(a=a.reshape(5 * n_sets, u), s=s.reshape(5 * n_sets, u))
    for g, index in (("a", a), ("s", s)):
        groups[g] = cell_columns(tm.gather(tables_fr, index[:, :, below], len(below)).reshape(5 * n_sets, len(below), 32), k, below)
    if lookup_z:
        z = gm.grand_product(tables_fr, inputs, a, s, beta, gamma, pad_row, rows=u)
        facts["grand_report"] = gm.report(z, u)
        groups["zlookup"] = [col + [None] * (n - u - 1) for st in z for col in st]
    else:
        groups["zlookup"] = [[0] * (u + 1) + [None] * (n - u - 1) for _ in range(5 * n_sets)]
    assert {g: len(v) for g, v in groups.items()} == qm.group_columns(n_sets, chunk_len)
    return blind_groups(groups, u), facts
