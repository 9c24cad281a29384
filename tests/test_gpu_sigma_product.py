"""aesw_sigma_product_device / Context.permutation_product on the GPU over synthetic columns and mappings (tests/sigma_cases.py:
sc.PRODUCTS, sc.STORE_MODES), against tests/sigma_model.py in Python integers: every written cell of Z, every closing cell, the
report, and the poison (tests/guarded.py) above row min(n_rows, 2^k - 1) and in the guard bands.  The mapping is a random
partition of the cells in the rows below n_rows into cycles, with bytes constant on each cycle, and the identity at and above
n_rows -- so the product closes, and one changed byte opens it.  The columns are split over an advice and a fixed buffer and
chosen through d_source in a shuffled order.  Planted: a zero term, a mapping entry and a source entry out of range, a beta and
a gamma that are not canonical; every refusal leaves the outputs untouched."""
import numpy as np
import pytest

import guarded as G
import sigma_cases as sc
import sigma_model as sm

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1
BETA, GAMMA = (sc.seeded(s) for s in sc.CHALLENGE_SEEDS)

_tables = {}


world = sc.world  # the synthetic columns and mappings, shared with tests/test_gpu_sigma_reach.py and tests/test_sigma_model.py


def tables(ctx, k, n_cols):
    if (k, n_cols) not in _tables:
        _tables[k, n_cols] = ctx.permutation_tables(k, n_cols)
    return _tables[k, n_cols]


def cell(value):
    import torch
    return torch.from_numpy(np.frombuffer(int(value).to_bytes(32, "little"), np.uint8).copy()).cuda()


def mont(value):
    return value * sm.M % sm.R


def product(pkg, ctx, arena, shape, buffers, source, mapping, beta_cell, gamma_cell, expect=OK, over=None, n_fixed=None):
    """The C call on guarded outputs: the last n_fixed buffers are the fixed ones (default: one, where there are two)."""
    import torch
    k, n_cols, chunk_len, n_rows = shape
    lib = pkg.api.load_sigma_library()
    sets = -(-n_cols // chunk_len)
    n_fixed = (1 if len(buffers) > 1 else 0) if n_fixed is None else n_fixed
    n_advice = len(buffers) - n_fixed
    d_adv = torch.from_numpy(np.ascontiguousarray(buffers[:n_advice])).cuda() if n_advice else None
    d_fix = torch.from_numpy(np.ascontiguousarray(buffers[n_advice:])).cuda() if n_fixed else None
    d_src = torch.from_numpy(source.astype(np.uint32).view(np.int32)).cuda()
    d_map = torch.from_numpy(np.ascontiguousarray(mapping, np.uint32).view(np.int32)).cuda()
    z = arena.out("z", (sets * 32) << k, (sets, 1 << k, 32))
    closing = arena.out("closing", sets * 32, (sets, 32))
    rep = arena.out("report", 48)
    ws = arena.out("workspace", int(lib.aesw_sigma_workspace_bytes(k, n_cols, chunk_len)))
    t = tables(ctx, k, n_cols)
    args = dict(h=ctx._h, k=k, n_cols=n_cols, chunk_len=chunk_len, u=n_rows, adv=d_adv.data_ptr() if n_advice else None, n_adv=n_advice,
                fix=d_fix.data_ptr() if n_fixed else None, n_fix=n_fixed, src=d_src.data_ptr(), map=d_map.data_ptr(), tables=t.data_ptr(), beta=beta_cell.data_ptr(),
                gamma=gamma_cell.data_ptr(), z=z.data_ptr(), closing=closing.data_ptr(), ws=ws.data_ptr(), rep=rep.data_ptr())
    args.update(over or {})
    rc = lib.aesw_sigma_product_device(*[args[a] for a in ("h", "k", "n_cols", "chunk_len", "u", "adv", "n_adv", "fix", "n_fix", "src", "map", "tables", "beta", "gamma",
                                                           "z", "closing", "ws", "rep")], ctx._stream())
    assert rc == expect, (rc, ctx._lib.aesw_last_error(ctx._h))
    torch.cuda.synchronize()
    return z, closing, rep


def held(pkg, arena, shape, got, model, what):
    """Z, the closing cells and the report against the model; the poison above the last written row and in the bands"""
    import torch
    k, _n_cols, _chunk_len, n_rows = shape
    z, closing, rep = got
    exp_z, exp_closing = sm.z_cells(model[0], n_rows, k)
    last = min(n_rows, (1 << k) - 1)
    dev = z[:, :last + 1].cpu().numpy()
    bad = np.argwhere((dev != exp_z).any(axis=2))
    assert not bad.size, "%r: %d cells of Z differ, first (set, row) %r" % (what, len(bad), bad[0].tolist())
    assert last == (1 << k) - 1 or arena.poisoned_on_device(z[:, last + 1:]), "%r: a row above the closing product was written" % (what,)
    assert np.array_equal(closing.cpu().numpy(), exp_closing), what
    report = pkg.api.sigma_report_dict(rep.view(torch.int64))
    assert report == model[1], (what, report, model[1])
    arena.check_on_device()
    return report


@pytest.mark.parametrize("shape", sc.PRODUCTS, ids=lambda s: "k%d-c%d-l%d-u%d" % s)
def test_z_the_closing_cells_and_the_report_are_the_models(pkg, ctx, shape):
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x7369 + sc.PRODUCTS.index(shape))
    model = sm.product(k, list(columns), mapping, BETA, GAMMA, chunk_len, n_rows)
    arena = G.DeviceArena(G.CANARIES[sc.PRODUCTS.index(shape) % 2])
    got = product(pkg, ctx, arena, shape, buffers, source, mapping, cell(mont(BETA)), cell(mont(GAMMA)))
    report = held(pkg, arena, shape, got, model, shape)
    assert report == {"sets": -(-n_cols // chunk_len), "open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}
    assert bytes(got[0][0, 0].cpu().numpy()) == sm.ONE_CELL and bytes(got[1][-1].cpu().numpy()) == sm.ONE_CELL
    # one byte changed in a cycle of more than one cell opens the argument
    c, i = next((c, i) for c in range(n_cols) for i in range(n_rows) if mapping[c, i] != c * (1 << k) + i) if n_cols * n_rows > 3 else (None, None)
    if c is not None:
        changed = columns.copy()
        changed[c, i] ^= 0x40
        b2 = np.empty_like(changed)
        b2[source] = changed
        model = sm.product(k, list(changed), mapping, BETA, GAMMA, chunk_len, n_rows)
        assert model[1]["open"]
        arena = G.DeviceArena()
        held(pkg, arena, shape, product(pkg, ctx, arena, shape, b2, source, mapping, cell(mont(BETA)), cell(mont(GAMMA))), model, ("changed", shape))


@pytest.mark.parametrize("mode", sc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(pkg, ctx, mode):
    shape = sc.STORE_SHAPE
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x736d)
    model = sm.product(k, list(columns), mapping, BETA, GAMMA, chunk_len, n_rows)
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[mode % 2])
        got = product(pkg, ctx, arena, shape, buffers, source, mapping, cell(mont(BETA)), cell(mont(GAMMA)))
    finally:
        ctx.set_option("fr_store_mode", before)
    assert not held(pkg, arena, shape, got, model, ("mode", mode))["open"]


def test_a_planted_zero_term_zeroes_z_behind_it_in_its_set_and_the_later_ones(pkg, ctx):
    shape = sc.ZERO_SHAPE
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x737a)
    c, i0 = sc.ZERO_CELL
    # The cell's image shares its byte, so the image's NUMERATOR is zero too: take a cell whose image lies behind it (a later row of
    # set 1, or set 2), so that the zero denominator is what zeroes Z first.
    behind = lambda i: (int(mapping[c, i]) >> k) // chunk_len == 2 or ((int(mapping[c, i]) >> k) // chunk_len == 1 and (int(mapping[c, i]) & ((1 << k) - 1)) > i)  # noqa: E731
    i = next(i for i in range(i0, 2048) if i % 4 and behind(i))
    assert c // chunk_len == 1 and 1024 <= i < 2048 and i % 4
    m = int(mapping[c, i])
    lab = pow(sm.DELTA, m >> k, sm.R) * pow(sm.omega(k), m & ((1 << k) - 1), sm.R) % sm.R
    gamma = (-(int(columns[c, i]) + BETA * lab)) % sm.R
    model = sm.product(k, list(columns), mapping, BETA, gamma, chunk_len, n_rows)
    assert model[1]["zero_terms"] == 1 and model[1]["first_zero"] == (1 << k) + i and model[1]["open"]
    assert all(model[0][1][: i + 1]) and not any(model[0][1][i + 1:]) and not any(model[0][2]) and all(model[0][0])  # the model says so
    arena = G.DeviceArena()
    got = product(pkg, ctx, arena, shape, buffers, source, mapping, cell(mont(BETA)), cell(mont(gamma)))
    held(pkg, arena, shape, got, model, "zero term")
    z, closing, _ = got
    assert z[1, i].any() and not z[1, i + 1:n_rows + 1].any() and not z[2, :n_rows + 1].any() and not closing[1:].any() and closing[0].any()


def test_entries_out_of_range_read_as_the_cell_itself_and_as_zero_bytes(pkg, ctx):
    shape = (11, 5, 2, (1 << 11) - 6)
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x736f)
    mapping = mapping.copy()
    mapping[3, 1500] = n_cols * (1 << k) + 5
    mapping[4, 2044] = 0xFFFFFFFF  # at a row behind n_rows: neither read nor counted
    model = sm.product(k, list(columns), mapping, BETA, GAMMA, chunk_len, n_rows)
    assert model[1]["out_of_range"] == 1
    arena = G.DeviceArena()
    held(pkg, arena, shape, product(pkg, ctx, arena, shape, buffers, source, mapping, cell(mont(BETA)), cell(mont(GAMMA))), model, "mapping out of range")
    # a source entry behind the buffers: that column reads as zero bytes
    src = source.copy()
    src[2] = n_cols
    cols = list(columns)
    cols[2] = None
    model = sm.product(k, cols, mapping, BETA, GAMMA, chunk_len, n_rows)
    model[1]["out_of_range"] += 1
    arena = G.DeviceArena()
    held(pkg, arena, shape, product(pkg, ctx, arena, shape, buffers, src, mapping, cell(mont(BETA)), cell(mont(GAMMA))), model, "source out of range")


@pytest.mark.parametrize("which", ("beta", "gamma"))
def test_a_challenge_that_is_not_canonical_zeroes_every_written_cell(pkg, ctx, which):
    shape = (11, 4, 3, 1025)
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x736e)
    raw = sc.NONCANONICAL[which == "gamma"]
    beta, gamma = (raw, GAMMA) if which == "beta" else (BETA, raw)
    model = sm.product(k, list(columns), mapping, beta, gamma, chunk_len, n_rows)
    assert model[1]["noncanonical"]
    arena = G.DeviceArena()
    got = product(pkg, ctx, arena, shape, buffers, source, mapping, cell(raw if which == "beta" else mont(BETA)), cell(raw if which == "gamma" else mont(GAMMA)))
    held(pkg, arena, shape, got, model, which)
    assert not got[0][:, :n_rows + 1].any() and not got[1].any()


def test_the_python_face_and_the_refusals(pkg, ctx):
    import torch
    shape = (10, 4, 3, 1000)
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(k, n_cols, n_rows, 0x7370)
    model = sm.product(k, list(columns), mapping, BETA, GAMMA, chunk_len, n_rows)
    exp_z, exp_closing = sm.z_cells(model[0], n_rows, k)
    t = tables(ctx, k, n_cols)
    adv, fix = torch.from_numpy(buffers[:3].copy()).cuda(), torch.from_numpy(buffers[3:].copy()).cuda()
    z, closing, rep = ctx.permutation_product(k, n_cols, chunk_len, adv, fix, source, mapping, t, BETA, GAMMA, n_rows=n_rows)
    assert np.array_equal(z[:, :n_rows + 1].cpu().numpy(), exp_z) and np.array_equal(closing.cpu().numpy(), exp_closing) and rep == model[1]
    d_map = torch.from_numpy(mapping.view(np.int32)).cuda()
    z2, _c, rep2 = ctx.permutation_product(k, n_cols, chunk_len, adv, fix, source, d_map, t, cell(mont(BETA)), cell(mont(GAMMA)), n_rows=n_rows, sync=False)
    assert torch.equal(z2[:, :n_rows + 1], z[:, :n_rows + 1]) and pkg.api.sigma_report_dict(rep2) == model[1]
    arena = G.DeviceArena()
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    b, g = cell(mont(BETA)), cell(mont(GAMMA))
    outs = []
    for over, word in ((dict(k=9), "k must be"), (dict(k=29), "k must be"), (dict(n_cols=0), "n_cols"), (dict(n_cols=3075), "n_cols"), (dict(k=28, n_cols=17), "2^32"),
                       (dict(chunk_len=0), "chunk_len"), (dict(chunk_len=9), "chunk_len"), (dict(u=0), "n_rows"), (dict(u=(1 << k) + 1), "n_rows"),
                       (dict(adv=None), "d_advice"), (dict(adv=adv.data_ptr() + 4), "d_advice"), (dict(fix=None), "d_fixed"), (dict(fix=fix.data_ptr() + 8), "d_fixed"),
                       (dict(src=None), "d_source"), (dict(map=None), "d_map"), (dict(map=d_map.data_ptr() + 4), "d_map"), (dict(tables=None), "d_tables"),
                       (dict(beta=None), "d_beta"), (dict(gamma=b.data_ptr() + 8), "d_gamma"), (dict(z=None), "d_z_fr"), (dict(closing=None), "d_closing_fr"),
                       (dict(ws=None), "d_workspace"), (dict(rep=None), "d_report")):
        outs.extend(product(pkg, ctx, arena, shape, buffers, source, mapping, b, g, expect=INVALID, over=over))
        assert "aesw_sigma_product_device" in err() and word in err(), (over, err())
    group = pkg.Group([0])
    try:
        outs.extend(product(pkg, ctx, arena, shape, buffers, source, mapping, b, g, expect=INVALID, over=dict(h=group._h)))
        assert "aesw_sigma_product_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.permutation_product(k, n_cols, chunk_len, adv, fix, source, mapping, t, BETA, GAMMA)
    finally:
        group.close()
    arena.check_on_device()
    assert all(arena.poisoned_on_device(o) for o in outs)
    with pytest.raises(pkg.AeswError) as e:
        ctx.permutation_product(k, n_cols, chunk_len, adv, fix, source, mapping, t, BETA, GAMMA, n_rows=0)
    assert e.value.status == pkg.api.ERR_INVALID_ARG and "n_rows" in str(e.value)
    with pytest.raises(ValueError):
        ctx.permutation_product(k, n_cols, chunk_len, adv, fix, source, mapping[:3], t, BETA, GAMMA)
