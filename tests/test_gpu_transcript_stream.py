"""The op sequences of tests/transcript_cases.py on the GPU, through Context.transcript, against tests/transcript_model.py: every
block fill over 128 one-scalar calls, calls of more than two chunks (aesw_transcript_chunk_points / _scalars say how many that is),
squeezes at which the absorbed length is exactly one and two blocks -- the lazy last block -- each followed by a squeeze and by an
absorb, a squeeze as the very first op, the kinds and the write / common forms mixed, a proof buffer that ends inside an item
(between two sixteen-byte pieces and inside one), the identity first, last and twice, and init on a dirty state; calls of a chunk
and one item entered at every fill, a full block in front of the longest stream, calls of whole chunks, identities on both sides of a
chunk boundary, and points of which one coordinate alone is zero.  The state, the proof and every challenge are views of a guarded,
poisoned arena (tests/guarded.py); after every squeeze the challenge and the proof so far are the model's, byte for byte."""
import numpy as np
import pytest

import guarded as G
import transcript_cases as tc
import transcript_model as tm

pytestmark = pytest.mark.gpu


def _cases(pkg):
    lib = pkg.api.load_transcript_library()
    return tc.cases(int(lib.aesw_transcript_chunk_points()), int(lib.aesw_transcript_chunk_scalars()))


def run_case(pkg, ctx, case, canary):
    """the case on the device: (the model's transcript, its challenges, the device's challenges, the arena, the proof view, the Transcript)"""
    import torch
    arena = G.DeviceArena(canary)
    model, expected = tm.run(case.ops)
    capacity = len(model.proof) + 32 if case.capacity is None else case.capacity
    state, proof = arena.out("state", tm.STATE_BYTES), arena.out("proof", capacity)
    t = ctx.transcript(capacity, _state=state, _proof=proof)
    got, done = [], []
    for op in case.ops:
        name, items = op
        done.append(op)
        if name == "init":
            t.reset()
        elif name == "squeeze":
            out = arena.out("challenge", 32)
            assert t.squeeze(out=out) is out
            torch.cuda.synchronize()
            got.append(out.cpu().numpy().tobytes())
            so_far, challenges = tm.run(done)
            assert got[-1] == tm.challenge_cell(challenges[-1]).tobytes(), "challenge %d" % len(got)
            assert proof.cpu().numpy().tobytes() == tc.proof_buffer(done, capacity, canary), "the proof after challenge %d" % len(got)
        else:
            getattr(t, name)(torch.from_numpy(tc.item_bytes(name, items)).cuda())
    arena.check()
    assert len(got) == len(expected)
    return model, t, proof, capacity


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_a_sequence_of_ops_gives_the_models_challenges_proof_and_report(pkg, ctx, name):
    cases = _cases(pkg)
    case = cases[name]
    canary = G.CANARIES[sorted(cases).index(name) % 2]
    model, t, proof, capacity = run_case(pkg, ctx, case, canary)
    expected = model.status(capacity)
    assert t.status() == expected, name
    words = tm.state_words(t._state.cpu().numpy())
    count = (model.absorbed - 1) // tc.BLOCK * tc.BLOCK
    assert (words[8], words[25], words[30], words[31]) == (count, model.absorbed - count, model.points, 0), name
    if expected["proof_missed"]:
        with pytest.raises(pkg.AeswError, match="needs %d" % len(model.proof)) as e:
            t.proof()
        assert e.value.status == pkg.api.ERR_CAPACITY
    else:
        assert t.proof() == model.proof, name


def test_the_overflow_counts_what_did_not_fit_and_changes_no_challenge(pkg, ctx):
    cases = _cases(pkg)
    room = cases["overflow_with_room"]
    # the buffer ends between two sixteen-byte pieces, then inside one: 1 and 15 bytes of room in either piece of the third item
    for i, name in enumerate(["overflow"] + ["overflow_at_%d" % c for c in tc.CUT_INSIDE_A_PIECE]):
        cut = cases[name]
        assert cut.ops == room.ops
        model, t, proof, capacity = run_case(pkg, ctx, cut, G.CANARIES[i % 2])  # the guard band behind the short buffer is whole: run_case checks it
        assert capacity == cut.capacity and t.status()["proof_missed"] == len(model.proof) - capacity > tm.PROOF_ITEM, name
        assert proof.cpu().numpy().tobytes() == model.proof[:capacity], name
    _model, t_room, _proof, _capacity = run_case(pkg, ctx, room, G.CANARIES[1])  # the same challenges: every run is held to one model
    assert t_room.proof() == model.proof and t_room.status()["proof_missed"] == 0


def test_the_identity_is_counted_named_and_written_as_zeros(pkg, ctx):
    cases = _cases(pkg)
    chunk = int(pkg.api.load_transcript_library().aesw_transcript_chunk_points())
    for name, first, count in (("identity_first", 0, 1), ("identity_last", 6, 1), ("identity_twice", 2, 3), ("identity_across_chunks", 2 + chunk - 1, 3),
                               ("identity_in_the_second_chunk", 2 + 2 * chunk - 1, 2), ("half_identities", 5, 1)):
        model, t, _proof, _capacity = run_case(pkg, ctx, cases[name], G.CANARIES[0])
        st = t.status()
        assert (st["first_identity"], st["identities"]) == (first, count) == (model.first_identity, model.identities), name
        written = [i for op, items in cases[name].ops if op == "write_points" for i in items]
        zeros = [i for i, p in enumerate(written) if p is None]
        got = t.proof()
        assert zeros and all(got[32 * i:32 * i + 32] == bytes(32) for i in zeros) and all(got[32 * i:32 * i + 32] != bytes(32) for i in range(len(written)) if i not in zeros), name


def test_numpy_points_ints_and_device_cells_are_one_transcript(pkg, ctx):
    import torch
    pts, values = tc.points(3), tc.scalars(2)
    model = tm.Transcript().write_points(pts).write_scalars(values)
    expected = tm.challenge_cell(model.squeeze()).tobytes()
    cells = tc.item_bytes("write_scalars", values)
    for points, scalars in ((tc.item_bytes("write_points", pts), values), (torch.from_numpy(tc.item_bytes("write_points", pts)).cuda(), cells),
                            (tc.item_bytes("write_points", pts), torch.from_numpy(cells).cuda())):
        t = ctx.transcript(5 * 32)
        challenge = t.write_points(points).write_scalars(scalars).squeeze()
        assert tuple(challenge.shape) == (32,) and challenge.dtype == torch.uint8 and challenge.is_cuda
        assert challenge.cpu().numpy().tobytes() == expected and t.proof() == model.proof
    t = ctx.transcript()  # no proof buffer: challenges alone
    assert t.common_points(tc.item_bytes("write_points", pts)).common_scalars(values).squeeze().cpu().numpy().tobytes() == expected
    assert t.proof() == b"" and t.status() == {"proof_bytes": 0, "proof_missed": 0, "identities": 0, "first_identity": None}
    with pytest.raises(pkg.AeswError, match="proof_capacity=0"):
        t.write_points(tc.item_bytes("write_points", pts))
    assert np.array_equal(t._state.cpu().numpy()[26 * 8:30 * 8].view("<u8")[:3], np.zeros(3, "<u8"))
