"""aesw_theta_columns_device / Context.argument_columns on the GPU: the four columns commit_permuted commits to, for all
arguments at once (tests/theta_cases.py: tc.COLUMN_ROWS, tc.PAD_ROWS, tc.STORE_MODES).  The compressed tables the cells are
held against are tests/theta_model.py's, computed in Python integers; a cell below n_rows must be the model table's cell at the
index, every byte at and above n_rows must keep the poison (tests/guarded.py).  On the bytes the device wrote, per argument:
A'[0] == S'[0], A'[i] is S'[i] or A'[i - 1], A' is a permutation of the row-order input column and S' of the row-order table
column -- canonical cells are equal as integers exactly when their 32 bytes are equal."""
import numpy as np
import pytest

import guarded as G
import theta_cases as tc
import theta_model as tm

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
PACKED = 1
THETA = int.from_bytes(np.random.default_rng(tc.THETA_SEEDS[0]).bytes(40), "little") % tc.R

_worlds = {}


def world(pkg, ctx, oracle, k, n_sets, n):
    """The four index columns of one circuit on the device, and the model's compressed tables next to the device's."""
    import torch
    at = (k, n_sets, n)
    if at not in _worlds:
        rng = np.random.default_rng(100 * k + n)
        d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        d_pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
        mult, rep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n], PACKED)
        assert rep["misses"] == 0
        inputs, irep = ctx.lookup_inputs(k, n_sets, w, kw)
        assert irep == rep
        table = tm.compressed_tables(oracle.lookup_table(), THETA)
        d_table, trep = ctx.compress_table(THETA)
        assert not trep["noncanonical"] and np.array_equal(d_table.cpu().numpy(), table)
        _worlds[at] = {"mult": mult, "inputs": inputs, "table": torch.from_numpy(table).cuda(), "perm": {}}
    return _worlds[at]


def permuted(ctx, wd, k, n_sets, u, pad):
    if (u, pad) not in wd["perm"]:
        a, s, rep = ctx.permuted_columns(k, n_sets, wd["mult"], n_rows=u, pad_row=pad)
        assert rep["overflowed"] == 0
        wd["perm"][(u, pad)] = (a, s)
    return wd["perm"][(u, pad)]


def expected(torch, table, index, k, n_sets, u, pad):
    """uint8 [n_sets, 5, u, 32] on the device: the model's table of each argument's arity, indexed"""
    if index is None:
        idx = torch.from_numpy(tm.table_column(u, pad)).cuda().expand(n_sets, 5, u)
    else:
        idx = index[:, :, :u].long() & 0xFFFFFFFF
    out = torch.zeros((n_sets, 5, u, 32), dtype=torch.uint8, device="cuda")
    for tag in tm.TAGS:
        i = idx[:, tag - 1]
        ok = i < tm.BINS
        out[:, tag - 1] = torch.where(ok[..., None], table[tm.TABLE_OF_TAG[tag]][i.clamp(max=tm.BINS - 1)], torch.zeros((), dtype=torch.uint8, device="cuda"))
    return out


def column(pkg, ctx, arena, name, index, table, k, n_sets, u, pad, expect=OK, over=None):
    import torch
    out = arena.out(name, (n_sets * 5 * 32) << k, (n_sets, 5, 1 << k, 32))
    args = dict(h=ctx._h, k=k, n_sets=n_sets, u=u, pad=pad, index=None if index is None else index.data_ptr(), table=table.data_ptr(), out=out.data_ptr())
    args.update(over or {})
    rc = pkg.api.load_theta_library().aesw_theta_columns_device(args["h"], args["k"], args["n_sets"], args["u"], args["pad"], args["index"], args["table"],
                                                                 args["out"], ctx._stream())
    assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
    torch.cuda.synchronize()
    return out


def four_columns(pkg, ctx, wd, arena, k, n_sets, u, pad, what):
    """inputs, table, A', S' as written, each checked cell for cell and for the poison behind n_rows"""
    import torch
    a, s = permuted(ctx, wd, k, n_sets, u, pad)
    got = {}
    for name, index in (("inputs", wd["inputs"]), ("table", None), ("a", a), ("s", s)):
        out = column(pkg, ctx, arena, name, index, wd["table"], k, n_sets, u, pad)
        exp = expected(torch, wd["table"], index, k, n_sets, u, pad)
        bad = torch.nonzero((out[:, :, :u] != exp).any(dim=3))
        assert not bad.numel(), "%s %r: %d cells differ, first (set, tag - 1, row) %r" % (name, what, len(bad), bad[0].tolist())
        assert u == 1 << k or arena.poisoned_on_device(out[:, :, u:]), "%s %r: a row at or behind n_rows was written" % (name, what)
        got[name] = out
    arena.check_on_device()
    return got


def multiset(torch, cells):
    """(the distinct cells, sorted; how often each occurs) of int64 [n, 4] cells"""
    return torch.unique(cells, dim=0, return_counts=True)


def relations(torch, got, whole_inputs, n_sets, k, u, what):
    """plookup's relations on the bytes.  A' permutes the argument's inputs over the u usable rows.  The circuit's own input
    column has 2^k rows, and a full set has lookups at and behind a small n_rows, so the relation is held against the WHOLE
    column `whole_inputs` (the inputs gathered over all 2^k rows) with 2^k - u cells of the all-zero row taken off: every row a
    prover cuts off to make room for blinding is a row whose selector is off.  No section of these circuits holds more than
    66 561 lookups, so the arrangement clips nothing (4.18) and the relation is asked of every argument."""
    zero = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    for st in range(n_sets):
        for tag in tm.TAGS:
            cells = {name: got[name][st, tag - 1, :u].contiguous().view(torch.int64) for name in got}  # [u, 4] words
            A, S = cells["a"], cells["s"]
            same_as_table = (A == S).all(dim=1)
            same_as_prev = torch.cat([torch.zeros(1, dtype=torch.bool, device="cuda"), (A[1:] == A[:-1]).all(dim=1)])
            assert bool(same_as_table[0]) and bool((same_as_table | same_as_prev).all()), (what, st, tag)
            x, y = multiset(torch, S), multiset(torch, cells["table"])
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), (what, st, tag, "S'")
            x, y = multiset(torch, A), multiset(torch, whole_inputs[st, tag - 1].contiguous().view(torch.int64))
            is_zero = (y[0] == zero).all(dim=1)
            assert int(is_zero.sum()) == 1 and int(y[1][is_zero]) >= (1 << k) - u, (what, st, tag)
            counts = y[1] - is_zero.long() * ((1 << k) - u)
            keep = counts > 0
            assert torch.equal(x[0], y[0][keep]) and torch.equal(x[1], counts[keep]), (what, st, tag, "A'")


def whole_input_column(pkg, ctx, wd, k, n_sets):
    if "whole" not in wd:
        wd["whole"] = ctx.argument_columns(wd["inputs"], wd["table"], k, n_sets)
    return wd["whole"]


@pytest.mark.parametrize("n_sets,n", ((1, 95), (2, 120)))
@pytest.mark.parametrize("u", tc.COLUMN_ROWS)
def test_the_four_columns_cell_for_cell_and_their_relations(pkg, ctx, oracle, u, n_sets, n):
    import torch
    k = 17
    assert (n == pkg.block_capacity(k, n_sets)) == (n_sets == 1)
    wd = world(pkg, ctx, oracle, k, n_sets, n)
    at = tc.COLUMN_ROWS.index(u) + n_sets
    pad, mode = tc.PAD_ROWS[at % 2], tc.STORE_MODES[at % 3]
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        got = four_columns(pkg, ctx, wd, G.DeviceArena(G.CANARIES[at % 2]), k, n_sets, u, pad, (u, n_sets, pad, mode))
    finally:
        ctx.set_option("fr_store_mode", before)
    relations(torch, got, whole_input_column(pkg, ctx, wd, k, n_sets), n_sets, k, u, (u, n_sets))


@pytest.mark.parametrize("pad", tc.PAD_ROWS)
@pytest.mark.parametrize("mode", tc.STORE_MODES)
def test_every_store_mode_and_planted_indices_outside_the_table(pkg, ctx, oracle, mode, pad):
    import torch
    k, n_sets, u = 17, 1, 66563
    wd = world(pkg, ctx, oracle, k, n_sets, 95)
    index = wd["inputs"].clone()
    planted = {(0, 0, 0): 66561, (0, 1, 77): -1, (0, 2, u - 1): 66561, (0, 4, 4096): -1, (0, 3, 5): 66560}
    for at, v in planted.items():
        index[at] = v
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[mode % 2])
        out = column(pkg, ctx, arena, "planted", index, wd["table"], k, n_sets, u, pad)
        table_col = column(pkg, ctx, arena, "table", None, wd["table"], k, n_sets, u, pad)
    finally:
        ctx.set_option("fr_store_mode", before)
    assert torch.equal(out[:, :, :u], expected(torch, wd["table"], index, k, n_sets, u, pad)) and arena.poisoned_on_device(out[:, :, u:])
    assert torch.equal(table_col[:, :, :u], expected(torch, wd["table"], None, k, n_sets, u, pad)) and arena.poisoned_on_device(table_col[:, :, u:])
    for at in planted:
        assert not out[at].any(), at
    model = tm.compressed_tables(oracle.lookup_table(), THETA)  # the host's arithmetic once more, on the cells behind the table
    for tag in tm.TAGS:
        assert np.array_equal(table_col[0, tag - 1, tm.BINS:u].cpu().numpy(), np.broadcast_to(model[tm.TABLE_OF_TAG[tag]][pad], (u - tm.BINS, 32)))
    arena.check_on_device()


def test_a_larger_circuit_partly_filled(pkg, ctx, oracle):
    import torch
    k, n_sets, n, u = 18, 3, 420, (1 << 18) - 6
    assert n < pkg.block_capacity(k, n_sets)
    wd = world(pkg, ctx, oracle, k, n_sets, n)
    got = four_columns(pkg, ctx, wd, G.DeviceArena(), k, n_sets, u, 0, "k = 18")
    relations(torch, got, whole_input_column(pkg, ctx, wd, k, n_sets), n_sets, k, u, "k = 18")


def test_the_python_face_and_the_refusals(pkg, ctx, oracle):
    import torch
    k, n_sets, u = 17, 1, (1 << 17) - 6
    wd = world(pkg, ctx, oracle, k, n_sets, 95)
    out = ctx.argument_columns(wd["inputs"], wd["table"], k, n_sets, n_rows=u)
    assert torch.equal(out[:, :, :u], expected(torch, wd["table"], wd["inputs"], k, n_sets, u, 0))
    out = ctx.argument_columns(None, wd["table"], k, n_sets, pad_row=66560)
    assert torch.equal(out, expected(torch, wd["table"], None, k, n_sets, 1 << k, 66560))
    arena = G.DeviceArena()
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    outs = []
    for over, word in ((dict(k=16), "k must be"), (dict(k=31), "k must be"), (dict(n_sets=0), "n_sets"), (dict(n_sets=1025), "n_sets"), (dict(u=66560), "n_rows"),
                       (dict(u=(1 << 17) + 1), "n_rows"), (dict(pad=66561), "pad_row"), (dict(index=wd["inputs"].data_ptr() + 2), "d_index"), (dict(table=None), "d_table_fr"),
                       (dict(table=wd["table"].data_ptr() + 8), "d_table_fr"), (dict(out=None), "d_out_fr")):
        outs.append(column(pkg, ctx, arena, "refused", wd["inputs"], wd["table"], k, n_sets, u, 0, expect=INVALID, over=over))
        assert "aesw_theta_columns_device" in err() and word in err(), (over, err())
    group = pkg.Group([0])
    try:
        outs.append(column(pkg, ctx, arena, "refused", wd["inputs"], wd["table"], k, n_sets, u, 0, expect=INVALID, over=dict(h=group._h)))
        assert "aesw_theta_columns_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.argument_columns(None, wd["table"], k, n_sets)
    finally:
        group.close()
    arena.check_on_device()
    assert all(arena.poisoned_on_device(t) for t in outs)
    with pytest.raises(pkg.AeswError) as e:
        ctx.argument_columns(None, wd["table"], k, n_sets, n_rows=66560)
    assert e.value.status == pkg.api.ERR_INVALID_ARG and "n_rows" in str(e.value)
    with pytest.raises(ValueError):
        ctx.argument_columns(wd["inputs"][:, :4], wd["table"], k, n_sets)
