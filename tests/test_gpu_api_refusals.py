"""The marshalling helpers of api.py on the GPU, through every method written over them.

For each method one valid argument set at the smallest size its library takes, the outputs and the workspace in a guarded,
poisoned arena (tests/guarded.py): k = 10 with two columns for the transforms and the openings (k = 11 for the transform in
place: at k = 10 it needs no workspace), two points for evaluate, n_cols = 5 and chunk_len = 2 for the permutation argument and
sigma; the lookup family runs at k = 17, n_sets = 1 over four blocks, the smallest k whose rows hold the table (the libraries
refuse less), and the multiplicities are counted at the same k so that they feed it.

Per tensor argument one fault at a time -- no tensor, the wrong dtype on the device, the right dtype on the CPU, a view that is
not contiguous, the last dimension off by one, one byte short where a size is asked -- is refused with the class of
profiles/api_marshal/README.md in a text that names the argument.  Every refusal is raised in Python before any library call,
so the outputs still hold the poison afterwards; then the valid call runs once and the guards are intact.  Ints, numpy cells
and device cells for v, point and beta give the same bytes."""
import numpy as np
import pytest

import guarded as G

pytestmark = pytest.mark.gpu
PACKED = 1
K, N_SETS, N = 17, 1, 4
U = (1 << K) - 6
SK, N_COLS, CHUNK_LEN = 10, 5, 2   # the permutation argument and sigma
TK, T_COLS, N_POINTS = 10, 2, 2    # the transforms and the openings
TK_IN_PLACE = 11
THETA, BETA, GAMMA, V = 0x7468, 0x6265, 0x6761, 0x76


class Arg:
    """A tensor argument of a case: `like`, a valid device tensor the faults are cut from; `sized`: the argument is checked by
    its byte count, so its fault is one byte short; `free`: any shape goes (the index of gather_fr)."""

    def __init__(self, name, like, sized=False, free=False):
        self.name, self.like, self.sized, self.free = name, like, sized, free

    def faults(self, torch, other_device=None):
        t = self.like
        other = torch.int32 if t.dtype == torch.uint8 else torch.uint8
        wide = tuple(t.shape[:-1]) + (2 * t.shape[-1],)
        if other_device is not None:
            yield "on the other GPU", TypeError, torch.empty(t.shape, dtype=t.dtype, device=torch.device("cuda", other_device))
            return
        yield "no tensor", TypeError, object()
        yield "wrong dtype", TypeError, torch.empty(t.shape, dtype=other, device=t.device)
        yield "on the CPU", TypeError, torch.empty(t.shape, dtype=t.dtype)
        yield "not contiguous", ValueError, torch.empty(wide, dtype=t.dtype, device=t.device)[..., ::2]
        if self.sized:
            yield "one byte short", ValueError, torch.empty(t.numel() * t.element_size() - 1, dtype=torch.uint8, device=t.device)
        elif not self.free:
            yield "last dimension off by one", ValueError, torch.empty(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), dtype=t.dtype, device=t.device)


class Case:
    """call(**args) is the method; `tensors` maps the keys of args that are tensor arguments to their Arg; `outputs` are the
    keys whose tensors the call writes (views of `arena`), `in_place` those it overwrites."""

    def __init__(self, arena, call, args, tensors, outputs, in_place=()):
        self.arena, self.call, self.args, self.tensors, self.outputs, self.in_place = arena, call, args, tensors, outputs, in_place


def _cells(pkg, torch, values):
    return torch.from_numpy(pkg.api.cells_of([int(v) for v in values])).cuda()


def _columns(pkg, torch, k, n_cols, seed):
    rng = np.random.default_rng(seed)
    return _cells(pkg, torch, rng.integers(1, 1 << 62, n_cols << k)).view(n_cols, 1 << k, 32)


def _i32(arena, name, shape):
    import torch
    return arena.out(name, 4 * int(np.prod(shape))).view(torch.int32).view(shape)


def _u8(arena, name, shape):
    return arena.out(name, int(np.prod(shape)), tuple(shape))


def make_world(pkg, ctx):
    """What the lookup family reads, from the calls themselves: four blocks of a FixedAes128Config<17, 1> circuit."""
    import torch
    rng = np.random.default_rng(0x6d617273)
    d_key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    d_pt = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).cuda()
    w, kw = ctx.encrypt_witness(d_pt, d_key, PACKED), ctx.key_schedule_witness(d_key.reshape(1, 16), PACKED, want_rk=False)
    mult, rep = ctx.lookup_multiplicities(K, N_SETS, w, kw, [N], PACKED)
    assert rep["misses"] == 0
    a, s, prep = ctx.permuted_columns(K, N_SETS, mult, n_rows=U)
    assert prep["overflowed"] == 0
    inputs, _irep = ctx.lookup_inputs(K, N_SETS, w, kw)
    table, _trep = ctx.compress_table(THETA)
    inv, _vrep = ctx.invert_table(table, BETA, GAMMA)
    sigma_tables, ntt_tables = ctx.permutation_tables(SK, N_COLS), {k: ctx.ntt_tables(k) for k in (TK, TK_IN_PLACE)}
    mapping = np.arange(N_COLS << SK, dtype=np.uint32).reshape(N_COLS, 1 << SK)
    mapping[0, 1], mapping[3, 7] = mapping[3, 7], mapping[0, 1]  # one cycle of two cells; the bytes below are constant on it
    cell = {name: _cells(pkg, torch, [v])[0].contiguous() for name, v in (("theta", THETA), ("beta", BETA), ("gamma", GAMMA), ("v", V))}
    torch.cuda.synchronize()
    return dict(w=w, kw=kw, mult=mult, a=a, s=s, inputs=inputs, table=table, inv=inv, sigma_tables=sigma_tables, ntt_tables=ntt_tables, mapping=mapping,
                d_mapping=torch.from_numpy(mapping.view(np.int32)).cuda(), source=np.arange(N_COLS, dtype=np.uint32), cell=cell,
                columns=_columns(pkg, torch, TK, T_COLS, 0x636f), columns_in_place=_columns(pkg, torch, TK_IN_PLACE, T_COLS, 0x6970),
                advice=torch.full((N_COLS - 1, 1 << SK), 7, dtype=torch.uint8, device="cuda"), fixed=torch.full((1, 1 << SK), 7, dtype=torch.uint8, device="cuda"))


@pytest.fixture(scope="module")
def world(pkg, ctx):
    return make_world(pkg, ctx)


def _pair(method, **fixed):
    """A method whose _out is a pair, taken as _out0 and _out1"""
    return lambda _out0, _out1, **kw: method(_out=(_out0, _out1), **fixed, **kw)


def case_lookup_multiplicities(pkg, ctx, wd, arena):
    out = _i32(arena, "mult", (1, N_SETS, pkg.TABLE_ROWS))
    return Case(arena, lambda **kw: ctx.lookup_multiplicities(K, N_SETS, wd["w"], wd["kw"], [N], PACKED, **kw), dict(_out=out), dict(_out=Arg("_out", out)), ["_out"])


def case_permuted_columns(pkg, ctx, wd, arena):
    a, s = (_i32(arena, n, (N_SETS, 5, 1 << K)) for n in "as")
    return Case(arena, _pair(ctx.permuted_columns, k=K, n_sets=N_SETS, n_rows=U), dict(mult=wd["mult"][0], _out0=a, _out1=s),
                dict(mult=Arg("mult", wd["mult"][0]), _out0=Arg("_out", a), _out1=Arg("_out", s)), ["_out0", "_out1"])


def case_gather_fr(pkg, ctx, wd, arena):
    index, out = wd["a"][0, 0, :1 << 10], _u8(arena, "cells", (1 << 10, 32))
    return Case(arena, ctx.gather_fr, dict(index=index, table_fr=wd["table"][0], out=out),
                dict(index=Arg("index", index, free=True), table_fr=Arg("table_fr", wd["table"][0]), out=Arg("out", out, sized=True)), ["out"])


def case_compress_table(pkg, ctx, wd, arena):
    out = _u8(arena, "table_fr", pkg.api.TABLE_FR_SHAPE)
    return Case(arena, ctx.compress_table, dict(theta=wd["cell"]["theta"], _out=out), dict(theta=Arg("theta", wd["cell"]["theta"]), _out=Arg("_out", out)), ["_out"])


def case_lookup_inputs(pkg, ctx, wd, arena):
    out = _i32(arena, "inputs", (N_SETS, 5, 1 << K))
    return Case(arena, lambda **kw: ctx.lookup_inputs(K, N_SETS, wd["w"], wd["kw"], **kw), dict(_out=out), dict(_out=Arg("_out", out)), ["_out"])


def case_argument_columns(pkg, ctx, wd, arena):
    out = _u8(arena, "column", (N_SETS, 5, 1 << K, 32))
    return Case(arena, lambda **kw: ctx.argument_columns(k=K, n_sets=N_SETS, n_rows=U, **kw), dict(index=wd["inputs"], table_fr=wd["table"], out=out),
                dict(index=Arg("index", wd["inputs"]), table_fr=Arg("table_fr", wd["table"]), out=Arg("out", out)), ["out"])


def case_invert_table(pkg, ctx, wd, arena):
    out, c = _u8(arena, "inv_fr", pkg.api.INV_FR_SHAPE), wd["cell"]
    return Case(arena, ctx.invert_table, dict(table_fr=wd["table"], beta=c["beta"], gamma=c["gamma"], _out=out),
                dict(table_fr=Arg("table_fr", wd["table"]), beta=Arg("beta", c["beta"]), gamma=Arg("gamma", c["gamma"]), _out=Arg("_out", out)), ["_out"])


def case_grand_product(pkg, ctx, wd, arena):
    z, closing, c = _u8(arena, "z", (N_SETS, 5, 1 << K, 32)), _u8(arena, "closing", (N_SETS, 5, 32)), wd["cell"]
    ws = arena.out("workspace", int(pkg.api.load_grand_library().aesw_grand_workspace_bytes(K, N_SETS)))
    args = dict(inputs=wd["inputs"], a=wd["a"], s=wd["s"], table_fr=wd["table"], inv_fr=wd["inv"], beta=c["beta"], gamma=c["gamma"], _out0=z, _out1=closing, _workspace=ws)
    tensors = {n: Arg("_out" if n.startswith("_out") else n, t, sized=n == "_workspace") for n, t in args.items()}
    return Case(arena, _pair(ctx.grand_product, k=K, n_sets=N_SETS, n_rows=U), args, tensors, ["_out0", "_out1"])


def case_permutation_tables(pkg, ctx, wd, arena):
    out = _u8(arena, "tables", tuple(wd["sigma_tables"].shape))
    return Case(arena, lambda **kw: ctx.permutation_tables(SK, N_COLS, **kw), dict(_out=out), dict(_out=Arg("_out", out, sized=True)), ["_out"])


def case_permutation_product(pkg, ctx, wd, arena):
    import torch
    sets, c = -(-N_COLS // CHUNK_LEN), wd["cell"]
    z, closing = _u8(arena, "z", (sets, 1 << SK, 32)), _u8(arena, "closing", (sets, 32))
    ws = arena.out("workspace", int(pkg.api.load_sigma_library().aesw_sigma_workspace_bytes(SK, N_COLS, CHUNK_LEN)))
    d_source = torch.from_numpy(wd["source"].view(np.int32)).cuda()
    args = dict(advice_bytes=wd["advice"], fixed_bytes=wd["fixed"], source=d_source, mapping=wd["d_mapping"], tables=wd["sigma_tables"], beta=c["beta"], gamma=c["gamma"],
                _out0=z, _out1=closing, _workspace=ws)
    tensors = {n: Arg("_out" if n.startswith("_out") else n, t, sized=n in ("tables", "_workspace")) for n, t in args.items()}
    return Case(arena, _pair(ctx.permutation_product, k=SK, n_cols=N_COLS, chunk_len=CHUNK_LEN), args, tensors, ["_out0", "_out1"])


def case_ntt_tables(pkg, ctx, wd, arena):
    out = _u8(arena, "tables", tuple(wd["ntt_tables"][TK].shape))
    return Case(arena, lambda **kw: ctx.ntt_tables(TK, **kw), dict(_out=out), dict(_out=Arg("_out", out, sized=True)), ["_out"])


def _transform(name, call, k_out=TK):
    def case(pkg, ctx, wd, arena):
        out, tables = _u8(arena, "out", (T_COLS, 1 << k_out, 32)), wd["ntt_tables"][k_out]
        first = "ext" if name == "extended_to_coeff" else "cells" if name == "lagrange_to_coeff" else "coeff"
        return Case(arena, lambda **kw: call(ctx, kw.pop(first), **kw), {first: wd["columns"], "tables": tables, "out": out},
                    {first: Arg("cells", wd["columns"]), "tables": Arg("tables", tables, sized=True), "out": Arg("out", out)}, ["out"])
    return case


def case_lagrange_to_coeff_in_place(pkg, ctx, wd, arena):
    cells, tables = wd["columns_in_place"].clone(), wd["ntt_tables"][TK_IN_PLACE]
    ws = arena.out("workspace", int(pkg.api.load_ntt_library().aesw_ntt_workspace_bytes(TK_IN_PLACE, T_COLS)))
    return Case(arena, lambda **kw: ctx.lagrange_to_coeff(cells, TK_IN_PLACE, tables, out=cells, **kw), dict(_workspace=ws), dict(_workspace=Arg("_workspace", ws, sized=True)),
                [], in_place=[cells])


def case_permutation_columns_fr(pkg, ctx, wd, arena):
    out = _u8(arena, "sigma_fr", (N_COLS, 1 << SK, 32))
    return Case(arena, lambda **kw: ctx.permutation_columns_fr(SK, N_COLS, **kw), dict(mapping=wd["mapping"], sigma_tables=wd["sigma_tables"], _out=out),  # numpy: uploaded
                dict(mapping=Arg("mapping", wd["d_mapping"]), sigma_tables=Arg("sigma_tables", wd["sigma_tables"], sized=True), _out=Arg("_out", out)), ["_out"])


def _open_ws(pkg, arena, n_points):
    return arena.out("workspace", int(pkg.api.load_open_library().aesw_open_workspace_bytes(TK, T_COLS, n_points)))


def case_evaluate_columns(pkg, ctx, wd, arena):
    import torch
    points, out, ws = _cells(pkg, torch, [3, 5]), _u8(arena, "evals", (T_COLS, N_POINTS, 32)), _open_ws(pkg, arena, N_POINTS)
    args = dict(coeff=wd["columns"], points=points, out=out, _workspace=ws)
    return Case(arena, lambda **kw: ctx.evaluate_columns(k=TK, **kw), args, {n: Arg(n, t, sized=n == "_workspace") for n, t in args.items()}, ["out"])


def case_fold_columns(pkg, ctx, wd, arena):
    args = dict(coeff=wd["columns"], v=wd["cell"]["v"], acc=wd["columns"][1].clone(), out=_u8(arena, "folded", (1 << TK, 32)))
    return Case(arena, lambda **kw: ctx.fold_columns(k=TK, **kw), args, {n: Arg(n, t) for n, t in args.items()}, ["out"])


def case_divide_columns(pkg, ctx, wd, arena):
    args = dict(coeff=wd["columns"], point=wd["cell"]["v"], out=_u8(arena, "quot", (T_COLS, 1 << TK, 32)), _rem=_u8(arena, "rem", (T_COLS, 32)), _workspace=_open_ws(pkg, arena, 1))
    return Case(arena, lambda **kw: ctx.divide_columns(k=TK, **kw), args, {n: Arg(n, t, sized=n == "_workspace") for n, t in args.items()}, ["out", "_rem"])


def case_multiplicity_accumulator(pkg, ctx, wd, arena):
    out = _i32(arena, "mult", (N_SETS, pkg.TABLE_ROWS))
    return Case(arena, lambda **kw: ctx.multiplicity_accumulator(K, N_SETS, PACKED, **kw).reset(), dict(_out=out), dict(_out=Arg("_out", out)), ["_out"])


CASES = {
    "lookup_multiplicities": case_lookup_multiplicities, "permuted_columns": case_permuted_columns, "gather_fr": case_gather_fr,
    "compress_table": case_compress_table, "lookup_inputs": case_lookup_inputs, "argument_columns": case_argument_columns,
    "invert_table": case_invert_table, "grand_product": case_grand_product, "permutation_tables": case_permutation_tables,
    "permutation_product": case_permutation_product, "ntt_tables": case_ntt_tables,
    "lagrange_to_coeff": _transform("lagrange_to_coeff", lambda ctx, c, **kw: ctx.lagrange_to_coeff(c, TK, **kw)),
    "coeff_to_lagrange": _transform("coeff_to_lagrange", lambda ctx, c, **kw: ctx.coeff_to_lagrange(c, TK, **kw)),
    "coeff_to_extended": _transform("coeff_to_extended", lambda ctx, c, **kw: ctx.coeff_to_extended(c, TK, TK_IN_PLACE, **kw), TK_IN_PLACE),
    "extended_to_coeff": _transform("extended_to_coeff", lambda ctx, c, **kw: ctx.extended_to_coeff(c, TK, **kw)),
    "lagrange_to_coeff_in_place": case_lagrange_to_coeff_in_place, "permutation_columns_fr": case_permutation_columns_fr,
    "evaluate_columns": case_evaluate_columns, "fold_columns": case_fold_columns, "divide_columns": case_divide_columns,
    "multiplicity_accumulator": case_multiplicity_accumulator,
}


def _refused(case, other_device=None):
    """Every fault of every tensor argument is refused with its class, in a text that names the argument; how many were tried"""
    import torch
    tried = 0
    for key, arg in case.tensors.items():
        for fault, error, value in arg.faults(torch, other_device):
            with pytest.raises(error) as e:
                case.call(**dict(case.args, **{key: value}))
            assert arg.name in str(e.value), (key, fault, str(e.value))
            if fault in ("wrong dtype", "on the CPU", "on the other GPU"):
                assert "cuda:0" in str(e.value), (key, fault, str(e.value))
            tried += 1
    return tried


def _untouched(case, before):
    import torch
    torch.cuda.synchronize()
    for name in case.outputs:
        assert case.arena.poisoned_on_device(case.args[name]), "%s was written by a refused call" % name
    for t, b in zip(case.in_place, before):
        assert torch.equal(t, b), "a refused call in place wrote"


@pytest.mark.parametrize("method", sorted(CASES))
def test_every_fault_is_refused_before_anything_is_launched_and_the_valid_call_runs(pkg, ctx, world, method):
    case = CASES[method](pkg, ctx, world, G.DeviceArena(G.CANARIES[sorted(CASES).index(method) % 2]))
    before = [t.clone() for t in case.in_place]
    assert _refused(case) >= 4 * len(case.tensors)
    _untouched(case, before)
    case.call(**case.args)
    case.arena.check()
    for name in case.outputs:
        assert not case.arena.poisoned_on_device(case.args[name]), "%s was not written by the valid call" % name


@pytest.mark.parametrize("method", sorted(CASES))
def test_a_tensor_on_the_other_gpu_is_refused(pkg, ctx, world, method):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    case = CASES[method](pkg, ctx, world, G.DeviceArena())
    before = [t.clone() for t in case.in_place]
    assert _refused(case, other_device=1) == len(case.tensors)
    _untouched(case, before)


def test_the_forms_the_valid_calls_above_leave_out(pkg, ctx, world):
    """None for every output and workspace, numpy for source and mapping, index=None: the allocating half of the helpers"""
    import torch
    wd, c = world, world["cell"]
    z, closing, rep = ctx.permutation_product(SK, N_COLS, CHUNK_LEN, wd["advice"], wd["fixed"], wd["source"], wd["mapping"], wd["sigma_tables"], BETA, GAMMA)
    assert rep["open"] is False and rep["out_of_range"] == 0 and z.shape == (3, 1 << SK, 32) and closing.shape == (3, 32)
    z2, closing2, _rep = ctx.permutation_product(SK, N_COLS, CHUNK_LEN, wd["advice"], wd["fixed"], wd["source"], wd["d_mapping"], wd["sigma_tables"], c["beta"], c["gamma"])
    assert torch.equal(z, z2) and torch.equal(closing, closing2)
    assert torch.equal(ctx.permutation_columns_fr(SK, N_COLS, wd["mapping"], wd["sigma_tables"]), ctx.permutation_columns_fr(SK, N_COLS, wd["d_mapping"], wd["sigma_tables"]))
    column = ctx.argument_columns(None, wd["table"], K, N_SETS)
    assert column.shape == (N_SETS, 5, 1 << K, 32)
    assert torch.equal(ctx.gather_fr(wd["a"][0, 0, :64], wd["table"][0]), wd["table"][0][wd["a"][0, 0, :64].long()])
    in_place = wd["columns_in_place"].clone()
    assert ctx.lagrange_to_coeff(in_place, TK_IN_PLACE, wd["ntt_tables"][TK_IN_PLACE], out=in_place) is in_place
    assert torch.equal(in_place, ctx.lagrange_to_coeff(wd["columns_in_place"], TK_IN_PLACE, wd["ntt_tables"][TK_IN_PLACE]))
    quot, rem = ctx.divide_columns(wd["columns"], TK, V)
    assert quot.shape == wd["columns"].shape and torch.equal(rem, ctx.evaluate_columns(wd["columns"], TK, [V])[:, 0])


def test_ints_numpy_cells_and_device_cells_are_one_value(pkg, ctx, world):
    import torch
    wd, api = world, pkg.api
    np_cell, d_cell = api.fr_cell(V), world["cell"]["v"]
    folded = [ctx.fold_columns(wd["columns"], TK, v) for v in (V, np.int64(V), [V], np_cell, np_cell.reshape(1, 32), d_cell, d_cell.view(1, 32))]
    divided = [ctx.divide_columns(wd["columns"], TK, p) for p in (V, np_cell, d_cell)]
    evals = [ctx.evaluate_columns(wd["columns"], TK, p) for p in ([V, V + 1], np.stack([np_cell, api.fr_cell(V + 1)]), _cells(pkg, torch, [V, V + 1]))]
    inverted = [ctx.invert_table(wd["table"], b, GAMMA)[0] for b in (BETA, np.int64(BETA), wd["cell"]["beta"])]
    for same in (folded, [q for q, _r in divided], [r for _q, r in divided], evals, inverted + [wd["inv"]]):
        assert all(torch.equal(same[0], t) for t in same[1:])
    assert V + api.FR_MODULUS != V and torch.equal(ctx.fold_columns(wd["columns"], TK, V + api.FR_MODULUS), folded[0])  # reduced
    two = _cells(pkg, torch, [V, V])
    for cells in (two, [V, V], two.cpu().numpy()):
        with pytest.raises(ValueError, match="v must be one"):
            ctx.fold_columns(wd["columns"], TK, cells)
        with pytest.raises(ValueError, match="point must be one"):
            ctx.divide_columns(wd["columns"], TK, cells)
    # a challenge is an int or a device cell: a numpy cell is refused as it always was
    with pytest.raises(TypeError, match="beta"):
        ctx.invert_table(wd["table"], api.fr_cell(BETA), GAMMA)
    with pytest.raises(ValueError, match="points"):
        ctx.evaluate_columns(wd["columns"], TK, np.zeros((2, 31), np.uint8))
