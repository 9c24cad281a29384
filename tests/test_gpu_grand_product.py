"""aesw_grand_product_device / Context.grand_product on the GPU over synthetic index columns (tests/grand_cases.py:
gc.PRODUCT_ROWS, gc.PAD_ROWS, gc.STORE_MODES), against tests/grand_model.py in Python integers: every written cell of Z, the
closing cells, the report, and the poison (tests/guarded.py) above row min(n_rows, 2^k - 1) and in the guard bands.  k = 17, the
smallest k that holds the table.  The columns are seeded per argument -- so a carry that leaks across an argument or a set
shows -- and hold indices at and above the table's end and the miss marker; A' and S' draw from a pool of rows, which keeps the
model's inversions few.  Random columns close nowhere: every argument is open.  One case plants a zero denominator in the
middle of an argument: Z is zero from the next row on.  The inverse table is the device's own (tests/test_gpu_grand_invert.py
holds it against the model cell for cell); the model inverts for itself."""
import numpy as np
import pytest

import grand_cases as gc
import grand_model as gm
import guarded as G
import theta_model as tm

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
K = gc.K
ROWS = 1 << K
THETA = gc.seeded(gc.THETA_SEED)
BETA, GAMMA = (gc.seeded(s) for s in gc.CHALLENGE_SEEDS)
ZERO_AT = (0, 3, 70001)  # (set, tag, row) of the planted zero denominator: behind the table, inside a chunk, not at a lane's first row

_worlds = {}


def cell(value):
    import torch
    return torch.from_numpy(np.frombuffer(int(value * gm.M % gm.R).to_bytes(32, "little"), np.uint8).copy()).cuda()


def columns(n_sets, seed, rows=ROWS):
    """(inputs, a, s) int64 [n_sets, 5, rows]: inputs over the whole table, a and s from a pool of 3 000 rows per argument; planted in
    each: an index at the table's end, a large one and the miss marker (which read the all-zero row)."""
    rng = np.random.default_rng(seed)
    inputs = rng.integers(0, gm.BINS, (n_sets, 5, rows))
    a, s = np.empty_like(inputs), np.empty_like(inputs)
    for st in range(n_sets):
        for t in range(5):
            pool = rng.choice(gm.BINS, 3000, replace=False)
            a[st, t], s[st, t] = pool[rng.integers(0, 3000, rows)], pool[rng.integers(0, 3000, rows)]
            for col in (inputs, a, s):
                at = rng.integers(0, gm.BINS, 6)  # below every n_rows
                col[st, t, at[:2]], col[st, t, at[2:4]], col[st, t, at[4:]] = gm.BINS, 1 << 20, 0xFFFFFFFF
    return inputs, a, s


def compressed_table(oracle):
    """(host, device): the oracle's lookup table compressed under THETA, made once"""
    import torch
    if "table" not in _worlds:
        table = tm.compressed_tables(oracle.lookup_table(), THETA)
        _worlds["table"] = (table, torch.from_numpy(table).cuda())
    return _worlds["table"]


def world(pkg, ctx, oracle, name):
    """The columns of `name` on the device, the device's inverse table for their beta, and the model's Z per pad_row."""
    import torch
    table, d_table = compressed_table(oracle)
    if name not in _worlds:
        n_sets = 2 if name == "two_sets" else 1
        inputs, a, s = columns(n_sets, {"one_set": 0x6731, "two_sets": 0x6732, "zero": 0x6731}[name])
        beta = BETA
        if name == "zero":  # beta = -T_1[row]: the row leaves the pool of its argument and is planted once
            st, tag, at = ZERO_AT
            row = int(a[st, tag - 1, at])
            beta = (gm.R - gm.values(table[gm.TABLE_OF_TAG[tag]][row])[0]) % gm.R
            for col in (inputs, a, s):  # no other term of any argument is zero: the rows of a table compress to distinct cells
                col[col == row] = (row + 1) % gm.ZERO_ROW
            a[st, tag - 1, at] = row
        inv, rep = ctx.invert_table(d_table, beta, GAMMA)
        assert not rep["noncanonical"]
        dev = [torch.from_numpy(c.astype(np.uint32).view(np.int32)).cuda() for c in (inputs, a, s)]
        _worlds[name] = dict(n_sets=n_sets, host=(inputs, a, s), dev=dev, inv=inv, beta=beta, d_beta=cell(beta), d_gamma=cell(GAMMA), z={})
    w = _worlds[name]
    w["d_table"], w["table"] = d_table, table
    return w


def model(w, pad):
    if pad not in w["z"]:
        w["z"][pad] = gm.grand_product(w["table"], *w["host"], w["beta"], GAMMA, pad)
    return w["z"][pad]


def product(pkg, ctx, arena, w, n_rows, pad, expect=OK, over=None, k=K):
    import torch
    n_sets = w["n_sets"]
    lib = pkg.api.load_grand_library()
    z = arena.out("z", (n_sets * 5 * 32) << k, (n_sets, 5, 1 << k, 32))
    closing = arena.out("closing", n_sets * 5 * 32, (n_sets, 5, 32))
    rep = arena.out("report", 24)
    ws = arena.out("workspace", int(lib.aesw_grand_workspace_bytes(k, n_sets)))
    args = dict(h=ctx._h, k=k, n_sets=n_sets, u=n_rows, pad=pad, inputs=w["dev"][0].data_ptr(), a=w["dev"][1].data_ptr(), s=w["dev"][2].data_ptr(),
                table=w["d_table"].data_ptr(), inv=w["inv"].data_ptr(), beta=w["d_beta"].data_ptr(), gamma=w["d_gamma"].data_ptr(), z=z.data_ptr(),
                closing=closing.data_ptr(), ws=ws.data_ptr(), rep=rep.data_ptr())
    args.update(over or {})
    rc = lib.aesw_grand_product_device(*[args[n] for n in ("h", "k", "n_sets", "u", "pad", "inputs", "a", "s", "table", "inv", "beta", "gamma", "z", "closing", "ws", "rep")],
                                       ctx._stream())
    assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
    torch.cuda.synchronize()
    return z, closing, rep


def held(pkg, arena, w, got, n_rows, pad, what):
    """Z, the closing cells and the report against the model; the poison above the last written row"""
    import torch
    z, closing, rep = got
    exp_z, exp_closing = gm.z_cells(model(w, pad), n_rows, K)
    last = min(n_rows, ROWS - 1)
    bad = torch.nonzero((z[:, :, :last + 1] != torch.from_numpy(exp_z).cuda()).any(dim=3))
    assert not bad.numel(), "%r: %d cells of Z differ, first (set, tag - 1, row) %r" % (what, len(bad), bad[0].tolist())
    assert bytes(z[0, 0, 0].cpu().numpy()) == gm.ONE_CELL
    assert last == ROWS - 1 or arena.poisoned_on_device(z[:, :, last + 1:]), "%r: a row above the closing product was written" % (what,)
    assert np.array_equal(closing.cpu().numpy(), exp_closing), what
    words = [int(v) & (2 ** 64 - 1) for v in rep.view(torch.int64).tolist()]
    exp_rep = gm.report(model(w, pad), n_rows)
    assert pkg.api.grand_report_dict(rep.view(torch.int64)) == exp_rep, what
    arena.check_on_device()
    return words


@pytest.mark.parametrize("mode", gc.STORE_MODES)
@pytest.mark.parametrize("pad", gc.PAD_ROWS)
@pytest.mark.parametrize("n_rows", gc.PRODUCT_ROWS)
def test_z_the_closing_cells_and_the_report_are_the_models(pkg, ctx, oracle, n_rows, pad, mode):
    w = world(pkg, ctx, oracle, "one_set")
    at = gc.PRODUCT_ROWS.index(n_rows) + gc.PAD_ROWS.index(pad) + mode
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[at % 2])
        got = product(pkg, ctx, arena, w, n_rows, pad)
    finally:
        ctx.set_option("fr_store_mode", before)
    words = held(pkg, arena, w, got, n_rows, pad, (n_rows, pad, mode))
    assert words == [5, 5, 1]  # random columns close nowhere: every argument is open, the first is set 0, tag 1


def test_two_sets_with_columns_of_their_own_per_argument(pkg, ctx, oracle):
    w = world(pkg, ctx, oracle, "two_sets")
    n_rows, pad = gc.PRODUCT_ROWS[1], gc.PAD_ROWS[1]
    arena = G.DeviceArena()
    words = held(pkg, arena, w, product(pkg, ctx, arena, w, n_rows, pad), n_rows, pad, "two sets")
    assert words == [10, 10, 1]
    z = model(w, pad)
    assert len({arg[n_rows] for st in z for arg in st}) == 10  # no two arguments share a product: a leaked carry cannot hide


def test_a_zero_denominator_in_the_middle_zeroes_z_from_there_on(pkg, ctx, oracle):
    import torch
    w = world(pkg, ctx, oracle, "zero")
    st, tag, at = ZERO_AT
    n_rows, pad = gc.PRODUCT_ROWS[2], gc.PAD_ROWS[0]
    z = model(w, pad)[st][tag - 1]
    assert all(v != 0 for v in z[:at + 1]) and not any(z[at + 1:])  # the model says so
    arena = G.DeviceArena()
    got = product(pkg, ctx, arena, w, n_rows, pad)
    words = held(pkg, arena, w, got, n_rows, pad, "zero term")
    assert words == [5, 5, 1]
    dz = got[0][st, tag - 1]
    assert dz[at].any() and not dz[at + 1:n_rows + 1].any() and not got[1][st, tag - 1].any()
    assert bool(got[0][st, tag % 5, 1:n_rows + 1].view(torch.int64).reshape(-1, 4).any(dim=1).all())  # the next argument does not inherit it


def test_the_python_face_and_the_refusals(pkg, ctx, oracle):
    import torch
    w = world(pkg, ctx, oracle, "one_set")
    n_rows, pad = gc.PRODUCT_ROWS[2], gc.PAD_ROWS[0]
    exp_z, exp_closing = gm.z_cells(model(w, pad), n_rows, K)
    z, closing, rep = ctx.grand_product(K, 1, *w["dev"], w["d_table"], w["inv"], BETA, GAMMA, n_rows=n_rows, pad_row=pad)
    assert np.array_equal(z[:, :, :n_rows + 1].cpu().numpy(), exp_z) and np.array_equal(closing.cpu().numpy(), exp_closing)
    assert rep == {"arguments": 5, "open": 5, "first_open": (0, 1)}
    z2, _c, rep2 = ctx.grand_product(K, 1, *w["dev"], w["d_table"], w["inv"], w["d_beta"], w["d_gamma"], sync=False)  # n_rows = 2^k: the last row is Z[2^k - 1]
    assert torch.equal(z2[:, :, :n_rows + 1], z[:, :, :n_rows + 1]) and pkg.api.grand_report_dict(rep2)["arguments"] == 5
    arena = G.DeviceArena()
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    outs = []
    for over, word in ((dict(k=16), "k must be"), (dict(k=31), "k must be"), (dict(n_sets=0), "n_sets"), (dict(n_sets=1025), "n_sets"), (dict(u=66560), "n_rows"),
                       (dict(u=ROWS + 1), "n_rows"), (dict(pad=66561), "pad_row"), (dict(inputs=None), "d_in"), (dict(a=w["dev"][1].data_ptr() + 4), "d_a"),
                       (dict(s=None), "d_s"), (dict(table=None), "d_table_fr"), (dict(inv=w["inv"].data_ptr() + 8), "d_inv_fr"), (dict(beta=None), "d_beta"),
                       (dict(gamma=None), "d_gamma"), (dict(z=None), "d_z_fr"), (dict(closing=None), "d_closing_fr"), (dict(ws=None), "d_workspace"),
                       (dict(rep=None), "d_report")):
        outs.extend(product(pkg, ctx, arena, w, n_rows, pad, expect=INVALID, over=over))
        assert "aesw_grand_product_device" in err() and word in err(), (over, err())
    group = pkg.Group([0])
    try:
        outs.extend(product(pkg, ctx, arena, w, n_rows, pad, expect=INVALID, over=dict(h=group._h)))
        assert "aesw_grand_product_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.grand_product(K, 1, *w["dev"], w["d_table"], w["inv"], BETA, GAMMA)
    finally:
        group.close()
    arena.check_on_device()
    assert all(arena.poisoned_on_device(t) for t in outs)
    with pytest.raises(pkg.AeswError) as e:
        ctx.grand_product(K, 1, *w["dev"], w["d_table"], w["inv"], BETA, GAMMA, n_rows=66560)
    assert e.value.status == pkg.api.ERR_INVALID_ARG and "n_rows" in str(e.value)
    with pytest.raises(ValueError):
        ctx.grand_product(K, 1, w["dev"][0][:, :4], w["dev"][1], w["dev"][2], w["d_table"], w["inv"], BETA, GAMMA)
