"""Every refusal of libaesw_msm.so and of its Python face, in the manner of tests/test_gpu_api_refusals.py, whose Arg, Case and
checks this file takes as they are: per tensor argument of Context.msm_basis and Context.commit_columns one fault at a time -- no
tensor, the wrong dtype, on the CPU, not contiguous, the last dimension off by one, a workspace one byte short -- refused in Python
with the class of profiles/api_marshal/README.md in a text that names the argument; every refused size and pointer of the C ABI
with ERR_INVALID_ARG in a text that names the call and the argument.  Nothing is launched: the outputs and the workspace still hold
the poison afterwards.  Then the valid call runs once and the guards are intact."""
import numpy as np
import pytest

import guarded as G
import msm_cases as mc
import msm_model as mm
import test_gpu_api_refusals as ar

pytestmark = pytest.mark.gpu
K, N_COLS = 10, 2


def _world(pkg):
    import torch
    scalars = torch.from_numpy(np.stack([mm.scalar_cells(mc.fr_columns(K)[name]) for name in ("seeded", "ends")])).cuda()
    return dict(basis=torch.from_numpy(mc.basis_cells(K)).cuda(), scalars=scalars, canonical=torch.from_numpy(mm.canonical_points(mm.known_basis(1 << K))).cuda(),
                bytes=torch.from_numpy(np.stack([np.array(mc.byte_columns(K)[name], np.uint8) for name in ("seeded", "ends")])).cuda())


def case_commit_cells(pkg, ctx, wd, arena):
    ws = arena.out("workspace", int(pkg.api.load_msm_library().aesw_msm_workspace_bytes(K, N_COLS, mc.FR, 2)))
    args = dict(scalars=wd["scalars"], basis=wd["basis"], out=ar._u8(arena, "out", (N_COLS, 64)), _workspace=ws)
    return ar.Case(arena, lambda **kw: ctx.commit_columns(slices=2, **kw), args, {n: ar.Arg(n, t, sized=n == "_workspace") for n, t in args.items()}, ["out"])


def case_commit_bytes(pkg, ctx, wd, arena):
    ws = arena.out("workspace", int(pkg.api.load_msm_library().aesw_msm_workspace_bytes(K, N_COLS, mc.BYTES, 0)))
    args = dict(scalars=wd["bytes"], basis=wd["basis"], out=ar._u8(arena, "out", (N_COLS, 64)), _workspace=ws)
    return ar.Case(arena, ctx.commit_columns, args, {n: ar.Arg(n, t, sized=n == "_workspace") for n, t in args.items()}, ["out"])


def case_msm_basis(pkg, ctx, wd, arena):
    args = dict(points=wd["canonical"], out=ar._u8(arena, "basis", (1 << K, 64)), _report=ar._u8(arena, "report", (16,)))
    return ar.Case(arena, ctx.msm_basis, args, {n: ar.Arg(n, t) for n, t in args.items()}, ["out", "_report"])


CASES = {"commit_cells": case_commit_cells, "commit_bytes": case_commit_bytes, "msm_basis": case_msm_basis}


@pytest.mark.parametrize("method", sorted(CASES))
def test_every_fault_is_refused_before_anything_is_launched_and_the_valid_call_runs(pkg, ctx, method):
    case = CASES[method](pkg, ctx, _world(pkg), G.DeviceArena(G.CANARIES[sorted(CASES).index(method) % 2]))
    assert ar._refused(case) >= 4 * len(case.tensors)
    ar._untouched(case, [])
    case.call(**case.args)
    case.arena.check()
    for name in case.outputs:
        assert not case.arena.poisoned_on_device(case.args[name]), "%s was not written by the valid call" % name


def test_the_sizes_the_python_face_refuses(pkg, ctx):
    import torch
    wd = _world(pkg)
    with pytest.raises(pkg.AeswError, match="2\\^k points"):
        ctx.commit_columns(wd["scalars"][:, :512].contiguous(), wd["basis"][:512])  # k = 9
    with pytest.raises(pkg.AeswError, match="2\\^k points"):
        ctx.msm_basis(wd["canonical"][:1000])
    with pytest.raises(ValueError, match="scalars"):
        ctx.commit_columns(wd["scalars"][:, :512].contiguous(), wd["basis"])  # the rows of the columns are not the basis's
    with pytest.raises(ValueError, match="scalars"):
        ctx.commit_columns(wd["scalars"][0], wd["basis"])  # one column still has its leading dimension
    for slices in (65, -1, 1 << 32):
        with pytest.raises(pkg.AeswError, match="slices"):
            ctx.commit_columns(wd["scalars"], wd["basis"], slices=slices)
    with pytest.raises(pkg.AeswError, match="n_cols"):
        ctx.commit_columns(torch.empty((0, 1 << K), dtype=torch.uint8, device="cuda"), wd["basis"])


def test_every_refusal_of_the_c_abi_leaves_the_poison_whole(pkg, ctx):
    import torch
    lib, api = pkg.api.load_msm_library(), pkg.api
    wd = _world(pkg)
    arena = G.DeviceArena()
    out, report = arena.out("out", N_COLS * 64), arena.out("report", 16)
    big = arena.out("big", 64 << K)  # a basis to write, or something to overlap
    ws = arena.out("ws", int(lib.aesw_msm_workspace_bytes(K, N_COLS, mc.FR, 0)))
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    sc, b, c, o, r, g, w = wd["scalars"].data_ptr(), wd["basis"].data_ptr(), wd["canonical"].data_ptr(), out.data_ptr(), report.data_ptr(), big.data_ptr(), ws.data_ptr()
    refusals = [
        # commit: k, n_cols, scalars, slices, d_scalars, d_basis, d_out, d_workspace
        ("commit", (9, N_COLS, 0, 0, sc, b, o, w), "k"), ("commit", (29, N_COLS, 0, 0, sc, b, o, w), "k"),
        ("commit", (K, 0, 0, 0, sc, b, o, w), "n_cols"), ("commit", (K, 65536, 0, 0, sc, b, o, w), "n_cols"),
        ("commit", (K, N_COLS, 2, 0, sc, b, o, w), "scalars"), ("commit", (K, N_COLS, 0, 65, sc, b, o, w), "slices"), ("commit", (K, N_COLS, 1, 65536, sc, b, o, w), "slices"),
        ("commit", (K, N_COLS, 0, 0, None, b, o, w), "d_scalars"), ("commit", (K, N_COLS, 0, 0, sc, None, o, w), "d_basis"),
        ("commit", (K, N_COLS, 0, 0, sc, b, None, w), "d_out"), ("commit", (K, N_COLS, 0, 0, sc, b, o, None), "d_workspace"),
        ("commit", (K, N_COLS, 0, 0, sc + 8, b, o, w), "d_scalars"), ("commit", (K, N_COLS, 0, 0, sc, b + 8, o, w), "d_basis"),
        ("commit", (K, N_COLS, 0, 0, sc, b, o + 4, w), "d_out"), ("commit", (K, N_COLS, 0, 0, sc, b, o, w + 8), "d_workspace"),
        ("commit", (K, N_COLS, 0, 0, sc, g, g + 64, w), "d_out"),      # the commitments lie in the basis
        ("commit", (K, N_COLS, 1, 0, g, b, g + 64, w), "d_out"),       # ... and in the scalars
        ("commit", (K, N_COLS, 0, 0, sc, b, w + 64, w), "d_workspace"),  # the workspace overlaps the output
        ("commit", (K, N_COLS, 0, 0, sc, w + 128, o, w), "d_workspace"),  # ... and an input
        # basis: k, d_canonical, d_basis, d_report
        ("basis", (9, c, g, r), "k"), ("basis", (29, c, g, r), "k"),
        ("basis", (K, None, g, r), "d_canonical"), ("basis", (K, c, None, r), "d_basis"), ("basis", (K, c, g, None), "d_report"),
        ("basis", (K, c + 8, g, r), "d_canonical"), ("basis", (K, c, g + 8, r), "d_basis"), ("basis", (K, c, g, r + 4), "d_report"),
        ("basis", (K, w, w + 64, r), "d_basis"),                      # a partial overlap of the coordinates and the basis
        ("basis", (K, c, g, g + 64), "d_report"),                     # the report lies in the basis
    ]
    for f, args, word in refusals:
        assert getattr(lib, "aesw_msm_%s_device" % f)(ctx._h, *args, s) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_msm_%s_device" % f) in err() and word in err(), (f, args, err())
    assert lib.aesw_msm_commit_device(None, K, N_COLS, 0, 0, sc, b, o, w, s) == api.ERR_INVALID_ARG
    assert lib.aesw_msm_basis_device(None, K, c, g, r, s) == api.ERR_INVALID_ARG
    torch.cuda.synchronize()
    arena.check()
    assert all(arena.poisoned_on_device(t) for t in (out, report, big, ws))
