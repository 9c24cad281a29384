"""Every refusal of libaesw_transcript.so and of its Python face, in the manner of tests/test_gpu_msm_refusals.py, whose Arg, Case
and checks (tests/test_gpu_api_refusals.py) this file takes as they are: per tensor argument of Context.transcript and of the
methods of Transcript one fault at a time -- no tensor, the wrong dtype, on the CPU, not contiguous, the last dimension off by one
-- refused in Python with the class of profiles/api_marshal/README.md in a text that names the argument; every refused size and
pointer of the C ABI with ERR_INVALID_ARG in a text that names the call and the argument; a Group.  Nothing is launched: the state,
the proof and the challenge still hold the poison afterwards.  Then the valid calls run once, the guards are intact and the
challenge is the model's."""
import numpy as np
import pytest

import guarded as G
import test_gpu_api_refusals as ar
import transcript_cases as tc
import transcript_model as tm

pytestmark = pytest.mark.gpu
N = 3
CAPACITY = N * tm.PROOF_ITEM


def _world():
    import torch
    return dict(points=torch.from_numpy(tc.item_bytes("write_points", tc.points(N))).cuda(), cells=torch.from_numpy(tc.item_bytes("write_scalars", tc.scalars(N))).cuda())


def _transcript(ctx, arena):
    """a Transcript on a guarded state and proof, poisoned again after the constructor's init"""
    import torch
    state, proof = ar._u8(arena, "state", (tm.STATE_BYTES,)), ar._u8(arena, "proof", (CAPACITY,))
    t = ctx.transcript(CAPACITY, _state=state, _proof=proof)
    torch.cuda.synchronize()
    arena.repoison()
    return t, state, proof


def case_constructor(ctx, wd, arena):
    args = dict(_state=ar._u8(arena, "state", (tm.STATE_BYTES,)), _proof=ar._u8(arena, "proof", (CAPACITY,)))
    return ar.Case(arena, lambda **kw: ctx.transcript(CAPACITY, **kw), args, {n: ar.Arg(n, t) for n, t in args.items()}, ["_state", "_proof"]), None, ["_state"]


def _method(name, key):
    def case(ctx, wd, arena):
        t, state, proof = _transcript(ctx, arena)
        args = {key: wd[key], "_state": state, "_proof": proof}
        call = lambda _state, _proof, **kw: getattr(t, name)(**kw)  # noqa: E731
        written = ["_state", "_proof"] if name.startswith("write") else ["_state"]
        return ar.Case(arena, call, args, {key: ar.Arg(key, wd[key])}, ["_state", "_proof"]), t, written
    return case


def case_squeeze(ctx, wd, arena):
    t, state, proof = _transcript(ctx, arena)
    args = dict(out=ar._u8(arena, "challenge", (32,)), _state=state, _proof=proof)
    return ar.Case(arena, lambda _state, _proof, **kw: t.squeeze(**kw), args, dict(out=ar.Arg("out", args["out"])), ["out", "_state", "_proof"]), t, ["out", "_state"]


CASES = {"constructor": case_constructor, "common_points": _method("common_points", "points"), "write_points": _method("write_points", "points"),
         "common_scalars": _method("common_scalars", "cells"), "write_scalars": _method("write_scalars", "cells"), "squeeze": case_squeeze}


@pytest.mark.parametrize("method", sorted(CASES))
def test_every_fault_is_refused_before_anything_is_launched_and_the_valid_call_runs(pkg, ctx, method):
    import torch
    arena = G.DeviceArena(G.CANARIES[sorted(CASES).index(method) % 2])
    case, t, written = CASES[method](ctx, _world(), arena)
    assert ar._refused(case) >= 4 * len(case.tensors)
    ar._untouched(case, [])
    if t is not None:
        t.reset()  # the faults ran against a state that still held the poison
    result = case.call(**case.args)
    torch.cuda.synchronize()
    arena.check()
    for name in case.outputs:
        assert arena.poisoned_on_device(case.args[name]) == (name not in written), name
    model = tm.Transcript()
    if method == "squeeze":
        assert result.cpu().numpy().tobytes() == tm.challenge_cell(model.squeeze()).tobytes()
    elif method != "constructor":
        getattr(model, method)(tc.points(N) if "points" in method else tc.scalars(N))
        assert t.squeeze().cpu().numpy().tobytes() == tm.challenge_cell(model.squeeze()).tobytes() and t.proof() == model.proof


def test_the_sizes_the_library_refuses_through_the_python_face(pkg, ctx):
    import torch
    t = ctx.transcript(CAPACITY)
    for n in (0, 65536):
        for call, shape in ((t.write_points, (n, 64)), (t.common_points, (n, 64)), (t.write_scalars, (n, 32)), (t.common_scalars, (n, 32))):
            with pytest.raises(pkg.AeswError, match="n must be 1 ... 65535") as e:
                call(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
            assert e.value.status == pkg.api.ERR_INVALID_ARG
    assert t.status() == {"proof_bytes": 0, "proof_missed": 0, "identities": 0, "first_identity": None}
    with pytest.raises(pkg.AeswError):
        pkg.Group.transcript(None)


def test_every_refusal_of_the_c_abi_leaves_the_poison_whole(pkg, ctx):
    import torch
    lib, api = pkg.api.load_transcript_library(), pkg.api
    wd = _world()
    arena = G.DeviceArena()
    state, proof, challenge = arena.out("state", tm.STATE_BYTES), arena.out("proof", CAPACITY), arena.out("challenge", 32)
    big = arena.out("big", 65536 * 64)  # items for the n that is too large, and something to overlap
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    st, pr, ch, p, c, g = state.data_ptr(), proof.data_ptr(), challenge.data_ptr(), wd["points"].data_ptr(), wd["cells"].data_ptr(), big.data_ptr()
    refusals = []
    for f, items, word in (("points", p, "d_points"), ("scalars", c, "d_cells")):
        refusals += [
            # d_state, n, the items, d_proof, proof_capacity
            (f, (st, 0, items, pr, CAPACITY), "n must"), (f, (st, 65536, g, pr, CAPACITY), "n must"), (f, (st, 0, items, None, 0), "n must"),
            (f, (None, N, items, pr, CAPACITY), "d_state"), (f, (st + 8, N, items, pr, CAPACITY), "d_state"),
            (f, (st, N, None, pr, CAPACITY), word), (f, (st, N, items + 8, pr, CAPACITY), word),
            (f, (st, N, items, pr + 8, CAPACITY), "d_proof"), (f, (st, N, items, pr, 0), "proof_capacity"), (f, (st, N, items, None, CAPACITY), "proof_capacity"),
            (f, (g, N, g + 64, pr, CAPACITY), "d_state must not overlap"),          # the state lies in the items
            (f, (st, N, g, g + 32, CAPACITY), "d_proof must not overlap"),          # the proof lies in the items
            (f, (g + 16, N, items, g, CAPACITY), "d_proof must not overlap"),       # ... and over the state
        ]
    for f, args, word in refusals:
        assert getattr(lib, "aesw_transcript_%s_device" % f)(ctx._h, *args, s) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_transcript_%s_device" % f) in err() and word in err(), (f, args, err())
    for f, args, word in (("init", (None,), "d_state"), ("init", (st + 4,), "d_state"), ("squeeze", (None, ch), "d_state"), ("squeeze", (st + 8, ch), "d_state"),
                          ("squeeze", (st, None), "d_challenge"), ("squeeze", (st, ch + 8), "d_challenge"), ("squeeze", (g, g + 240), "d_challenge must not overlap")):
        assert getattr(lib, "aesw_transcript_%s_device" % f)(ctx._h, *args, s) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_transcript_%s_device" % f) in err() and word in err(), (f, args, err())
    assert lib.aesw_transcript_init_device(None, st, s) == api.ERR_INVALID_ARG and lib.aesw_transcript_squeeze_device(None, st, ch, s) == api.ERR_INVALID_ARG
    assert lib.aesw_transcript_points_device(None, st, N, p, pr, CAPACITY, s) == api.ERR_INVALID_ARG
    assert lib.aesw_transcript_scalars_device(None, st, N, c, None, 0, s) == api.ERR_INVALID_ARG
    group = pkg.Group([0])
    try:
        for rc in (lib.aesw_transcript_init_device(group._h, st, s), lib.aesw_transcript_points_device(group._h, st, N, p, pr, CAPACITY, s),
                   lib.aesw_transcript_scalars_device(group._h, st, N, c, pr, CAPACITY, s), lib.aesw_transcript_squeeze_device(group._h, st, ch, s)):
            assert rc == api.ERR_INVALID_ARG
    finally:
        group.close()
    torch.cuda.synchronize()
    arena.check()
    assert all(arena.poisoned_on_device(t) for t in (state, proof, challenge, big))
    assert np.array_equal(wd["points"].cpu().numpy(), tc.item_bytes("write_points", tc.points(N)))
