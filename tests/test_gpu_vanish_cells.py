"""libaesw_vanish.so on the GPU against tests/quot_model.py, byte for byte, on poisoned, guard-banded buffers.

Every output cell at vc.FULL -- one and two column sets, both zetas, m = 4 and m = 8 -- over quot_model.seeded_columns; the stated
rows of vc.split_rows at vc.SPLIT, 2^15 rows, where the index of x_j's table carries; the tables and the scalars block cell for
cell; the three fr_store_modes; the accumulator against quotient_extended; a segment out of order."""
import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import quot_model as qm
import vanish_cases as vc
import vanish_gpu as vg
import vanish_model as vm

pytestmark = pytest.mark.gpu


def run_case(pkg, ctx, case, canary, seed=0x7663686c):
    """the whole fold through the accumulator, every output of the library guarded; returns (quotient, arena, tables, scalars)"""
    k, ext_k, zeta_sel, n_sets, chunk_len = case
    lib = pkg.api.load_vanish_library()
    cells, _values = vg.columns(ext_k, n_sets, chunk_len)
    d = vg.upload(cells)
    arena = G.DeviceArena(canary)
    tables = ctx.vanishing_tables(k, ext_k, zeta_sel, _out=arena.out("tables", int(lib.aesw_vanish_tables_bytes(k, ext_k))))
    scalars = ctx.vanishing_scalars(n_sets, chunk_len, *vg.challenges(seed), _out=arena.out("scalars", int(lib.aesw_vanish_scalars_bytes(n_sets, chunk_len))))
    acc = ctx.quotient_accumulator(k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), tables, scalars, _acc=arena.out("acc", 32 << ext_k, (1 << ext_k, 32)))
    values = [vg.put(arena, "values%d" % s, vg.values_of_set(cells, n_sets, chunk_len, s)) for s in range(acc.perm_sets)]
    out = vg.fold(ctx, acc, d, values, n_sets)
    arena.check()
    for g, t in d.items():
        G.assert_bytes("the %s columns are left alone" % g, t.cpu().numpy(), cells[g])
    return out, arena, tables, scalars


@pytest.mark.parametrize("case", vc.FULL, ids=lambda c: "k%d-e%d-z%d-n%d-l%d" % c)
def test_every_cell_of_the_quotient_is_the_model(pkg, ctx, case):
    k, ext_k, zeta_sel, n_sets, chunk_len = case
    out, _arena, tables, scalars = run_case(pkg, ctx, case, G.CANARIES[vc.FULL.index(case) % 2])
    G.assert_bytes("the quotient at %r" % (case,), out.cpu().numpy(), vg.expected(case))
    G.assert_bytes("the tables", tables.cpu().numpy().reshape(-1, 32), nm.to_cells(qm.tables(k, ext_k, zeta_sel)))
    G.assert_bytes("the scalars block", scalars.cpu().numpy().reshape(-1, 32), nm.to_cells(vm.scalars_block(n_sets, chunk_len, *vg.challenges())))
    sc = vm.scalars(n_sets, chunk_len, *vg.challenges())
    for name in pkg.api.VANISH_TABLES:  # vanishing_scalar finds every entry where the offset call says it lies
        for index, value in enumerate(sc[name]):
            assert nm.from_cells(ctx.vanishing_scalar(scalars, name, index).cpu().numpy()) == [value], (name, index)
    with pytest.raises(pkg.AeswError):
        ctx.vanishing_scalar(scalars, "y_pow", 3)


def test_the_stated_rows_where_the_table_index_carries(pkg, ctx):
    k, ext_k, _zeta_sel, _n_sets, _chunk_len = vc.SPLIT
    rows = vc.split_rows(k, ext_k)
    m, E = 1 << (ext_k - k), 1 << ext_k
    assert {0, 2 * m, E - 2 * m, E - 1, (1 << 14) - 1, 1 << 14, vc.BLIND * m - 1, vc.BLIND * m} <= set(rows) and len(rows) >= vc.SEEDED_ROWS
    out, _arena, _tables, _scalars = run_case(pkg, ctx, vc.SPLIT, G.CANARIES[0])
    import torch
    got = out[torch.as_tensor(rows, device=out.device)].cpu().numpy()
    G.assert_bytes("the quotient at the stated rows of %r" % (vc.SPLIT,), got, vg.expected(vc.SPLIT, rows=tuple(rows)))


@pytest.mark.parametrize("mode", vc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(pkg, ctx, mode):
    case = vc.FULL[0]
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        out, _arena, _tables, _scalars = run_case(pkg, ctx, case, G.CANARIES[mode % 2])
    finally:
        ctx.set_option("fr_store_mode", before)
    G.assert_bytes("the quotient under fr_store_mode %d" % mode, out.cpu().numpy(), vg.expected(case))


def test_the_accumulator_is_quotient_extended_and_follows_other_challenges(pkg, ctx):
    case, seed = vc.FULL[1], 0x6f746872
    k, ext_k, zeta_sel, n_sets, chunk_len = case
    cells, _values = vg.columns(ext_k, n_sets, chunk_len)
    d = vg.upload(cells)
    whole = ctx.quotient_extended(d, k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), *vg.challenges(seed))
    as_list = ctx.quotient_extended([d[g] for g in pkg.api.QUOTIENT_GROUPS], k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), *vg.challenges(seed),
                                    tables=ctx.vanishing_tables(k, ext_k, zeta_sel))
    stepped, _arena, _tables, _scalars = run_case(pkg, ctx, case, G.CANARIES[1], seed)
    G.assert_bytes("quotient_extended against the accumulator", whole.cpu().numpy(), stepped.cpu().numpy())
    G.assert_bytes("quotient_extended over a list of groups", as_list.cpu().numpy(), stepped.cpu().numpy())
    G.assert_bytes("the quotient under other challenges", stepped.cpu().numpy(), vg.expected(case, seed))
    assert not np.array_equal(vg.expected(case, seed), vg.expected(case))
    assert tuple(pkg.api.QUOTIENT_GROUPS) == qm.GROUPS
    with pytest.raises(ValueError):
        ctx.quotient_extended({g: t for g, t in d.items() if g != "l"}, k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), *vg.challenges(seed))
    with pytest.raises(ValueError):
        ctx.quotient_extended(dict(d, zperm=d["zperm"][:-1]), k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), *vg.challenges(seed))


def test_a_segment_out_of_order_or_given_twice_is_refused_and_acc_is_untouched(pkg, ctx):
    import torch
    k, ext_k, zeta_sel, n_sets, chunk_len = case = vc.FULL[0]
    lib = pkg.api.load_vanish_library()
    cells, _values = vg.columns(ext_k, n_sets, chunk_len)
    d = vg.upload(cells)
    arena = G.DeviceArena()
    tables, scalars = ctx.vanishing_tables(k, ext_k, zeta_sel), ctx.vanishing_scalars(n_sets, chunk_len, *vg.challenges())
    acc = ctx.quotient_accumulator(k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), tables, scalars, _acc=arena.out("acc", 32 << ext_k, (1 << ext_k, 32)))
    values = [torch.from_numpy(vg.values_of_set(cells, n_sets, chunk_len, s)).cuda() for s in range(acc.perm_sets)]
    lookup = (d["advice"][:3], d["selectors"][:5], d["table"], d["a"][:5], d["s"][:5], d["zlookup"][:5], d["l"])
    for wrong in (lambda: acc.permutation_set(0, values[0], d["sigma"][:3], d["zperm"][0], d["l"]), lambda: acc.lookup_set(0, *lookup), acc.divide):
        with pytest.raises(pkg.AeswError) as e:
            wrong()
        assert e.value.status == pkg.api.ERR_INVALID_ARG and "head(0) comes next" in str(e.value)
    torch.cuda.synchronize()
    assert arena.poisoned_on_device(acc.acc)
    acc.head(d["advice"][3 * n_sets], d["rcon"], d["zperm"], d["l"])
    for wrong in (lambda: acc.head(d["advice"][3 * n_sets], d["rcon"], d["zperm"], d["l"]), lambda: acc.permutation_set(1, values[1], d["sigma"][3:5], d["zperm"][1], d["l"])):
        with pytest.raises(pkg.AeswError):
            wrong()
    with pytest.raises(ValueError):  # set 0 holds three columns
        acc.permutation_set(0, values[1], d["sigma"][:3], d["zperm"][0], d["l"])
    acc.restart()
    out = vg.fold(ctx, acc, d, values, n_sets)
    with pytest.raises(pkg.AeswError) as e:
        acc.divide()
    assert "complete" in str(e.value)
    arena.check()
    G.assert_bytes("the fold after a restart", out.cpu().numpy(), vg.expected(case))
    for bad in ((9, 12, 1, 1, 3, 100), (10, 11, 1, 1, 3, 100), (10, 12, 2, 1, 3, 100), (10, 12, 1, 0, 3, 100), (10, 12, 1, 1, 4, 100), (10, 12, 1, 1, 3, 1024)):
        with pytest.raises(pkg.AeswError):
            ctx.quotient_accumulator(*bad, tables, scalars)
    assert int(lib.aesw_vanish_tables_bytes(10, 11)) == 0 and int(lib.aesw_vanish_scalars_bytes(0, 3)) == 0
