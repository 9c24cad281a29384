"""The specification of libaesw_transcript.so without a GPU.

tests/transcript_model.py -- halo2's Blake2b transcript over hashlib.blake2b, which implements the same function and keeps the lazy
last block itself -- is the reference.  csrc/aesw_transcript.h -- the state, the compression with its twelve unrolled rounds,
absorb with the lazy last block, finalize_copy, the messages, the compressed encoding, fr_from_u512 -- is compiled alone with g++
into tests/transcript_driver.cpp, a program of its own, once plain and once under -fsanitize=address,undefined, and held against
the model byte for byte: fr_from_u512 at its edges, the encodings of the generator, its negative, a point of either parity and the
identity, and every op sequence of tests/transcript_cases.py both item by item (n calls of halo2's method) and the way the absorb
kernel goes, chunk by chunk through transcript_stream_blocks; the two ways end in the same 256 bytes of state."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import msm_model as mm
import transcript_cases as tc
import transcript_model as tm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
OPS = {"init": 0, "common_points": 1, "write_points": 2, "common_scalars": 3, "write_scalars": 4, "squeeze": 5}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("transcript_driver")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = d / ("transcript_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "transcript_driver.cpp"), "-o", str(exes[name])], check=True)

    def run(*args, build="plain"):
        out = subprocess.run([str(exes[build])] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr[-2000:])
        return out.stdout.splitlines()
    run.dir = d
    return run


def script_bytes(ops):
    """the ops as the driver reads them, an init in front"""
    out = [struct.pack("<II", OPS["init"], 0)]
    for name, items in ops:
        out.append(struct.pack("<II", OPS[name], len(items) if items else 0))
        if items:
            out.append(tc.item_bytes(name, items).tobytes())
    return b"".join(out)


def expected_state_words(t, capacity):
    """what the model says of the state's words that are not the chain value or the block: count, fill and the report"""
    count = (t.absorbed - 1) // tc.BLOCK * tc.BLOCK if t.absorbed else 0
    st = t.status(capacity)
    return {8: count, 25: t.absorbed - count, 26: st["proof_bytes"], 27: st["proof_missed"], 28: st["identities"],
            29: (1 << 64) - 1 if st["first_identity"] is None else st["first_identity"], 30: t.points, 31: 0}


def test_the_header_is_free_of_hip_and_states_what_is_not_pinned():
    text = (CSRC / "aesw_transcript.h").read_text()
    assert "hip/" not in text and "asm" not in text and "__shared__" not in text
    assert '#include "aesw_fq.h"' in text and '#include "aesw_fr.h"' in text and text.count("#include \"aesw") == 2  # the two fields alone
    assert "parity with halo2 NOT PINNED" in text and "parity with halo2 NOT PINNED" in (ROOT / "include" / "aesw_transcript.h").read_text()
    assert "sigma[" not in text and "SIGMA[" not in text  # no schedule indexed at run time: the rounds are written out
    assert any("FR_R3" in line for line in text.split("static_assert")[1:])


def test_the_model_is_hashlib_with_the_lazy_last_block():
    import hashlib
    t = tm.Transcript().common_scalars([5])
    first = t.squeeze()
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
    h.update(b"\x02" + (5).to_bytes(32, "little") + b"\x00")
    assert first == int.from_bytes(h.digest(), "little") % tm.R and t.absorbed == 34
    h.update(b"\x00")
    assert t.squeeze() == int.from_bytes(h.digest(), "little") % tm.R  # the live state went on, with the first 0x00 absorbed
    g = mm.GENERATOR
    assert tm.point_message(g) == b"\x01" + b"\x01" + bytes(31) + b"\x02" + bytes(31) and tm.point_message(None) == b"\x01" + bytes(64)
    assert tm.point_compressed(g) == b"\x01" + bytes(31) and tm.point_compressed(mm.neg(g))[31] == 0x80 and tm.point_compressed(None) == bytes(32)
    for length in (tc.BLOCK, 2 * tc.BLOCK):
        ops = tc.absorbed_to(length)
        assert tm.run(ops)[0].absorbed == length and ops[-1] == tc.SQUEEZE and tm.run(ops[:-1])[0].absorbed == length - 1
        assert {name for name, _ in ops} == {"write_points", "common_scalars", "squeeze"}


def test_the_constants(drivers, pkg):
    chunk_points, chunk_scalars, point_message, scalar_message, item, state, most = [int(v) for v in drivers("constants")[0].split()]
    lib = pkg.api.load_transcript_library()
    assert chunk_points == int(lib.aesw_transcript_chunk_points()) and chunk_scalars == int(lib.aesw_transcript_chunk_scalars())
    assert (point_message, scalar_message, item, state, most) == (tm.POINT_MESSAGE, tm.SCALAR_MESSAGE, tm.PROOF_ITEM, tm.STATE_BYTES, 65535)
    assert state == pkg.api.TRANSCRIPT_STATE_BYTES
    long_calls = tc.cases(chunk_points, chunk_scalars)
    assert len(long_calls["points_in_one_call"].ops[0][1]) > 2 * chunk_points and len(long_calls["scalars_in_one_call"].ops[0][1]) > 2 * chunk_scalars


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_a_digest_reduces_to_its_cell_at_every_edge(drivers, build):
    d = drivers.dir
    r = tm.R
    halves = [(0, 0), ((1 << 256) - 1, (1 << 256) - 1), (r - 1, 0), (r, 0), (r + 1, 0), (0, 1), (0, r - 1)]
    raw = np.random.default_rng(0x7535313).bytes(64 * 200)
    values = [lo + (hi << 256) for lo, hi in halves] + [int.from_bytes(raw[64 * i:64 * i + 64], "little") for i in range(200)]
    (d / "digests.bin").write_bytes(b"".join(v.to_bytes(64, "little") for v in values))
    drivers("fr512", d / "digests.bin", d / "cells.bin", build=build)
    got = np.fromfile(d / "cells.bin", np.uint8).reshape(-1, 32)
    assert got.tobytes() == mm.scalar_cells([v % r for v in values]).tobytes()
    assert not got[0].any() and not got[3].any() and got[4].tobytes() == mm.scalar_cells([1])[0].tobytes()


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_the_encodings_of_the_special_points(drivers, build):
    d = drivers.dir
    g = mm.GENERATOR
    basis = mm.known_basis(64)
    even, odd = next(p for p in basis if p[1] % 2 == 0), next(p for p in basis if p[1] % 2 == 1)
    pts = [g, mm.neg(g), even, odd, None]
    mm.to_points(pts).tofile(d / "points.bin")
    drivers("encode", d / "points.bin", d / "messages.bin", d / "compressed.bin", build=build)
    assert (d / "messages.bin").read_bytes() == b"".join(tm.point_message(p) for p in pts)
    compressed = (d / "compressed.bin").read_bytes()
    assert compressed == b"".join(tm.point_compressed(p) for p in pts)
    assert [compressed[32 * i + 31] >> 7 for i in range(5)] == [0, 1, 0, 1, 0] and compressed[4 * 32:] == bytes(32)


@pytest.mark.parametrize("build", sorted(FLAGS))
@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_every_op_sequence_is_the_model_item_by_item_and_chunk_by_chunk(drivers, build, name):
    d = drivers.dir
    case = tc.cases()[name]
    t, challenges = tm.run(case.ops)
    capacity = len(t.proof) + 64 if case.capacity is None else case.capacity
    (d / "script.bin").write_bytes(script_bytes(case.ops))
    states = []
    for mode in ("items", "chunks"):
        drivers("script", mode, d / "script.bin", capacity, d / "proof.bin", d / "challenges.bin", d / "state.bin", build=build)
        proof = (d / "proof.bin").read_bytes()
        kept = min(len(t.proof), capacity)
        assert proof == tc.proof_buffer(case.ops, capacity, 0xa5) and proof[:kept] == t.proof[:kept], (name, mode)
        assert (d / "challenges.bin").read_bytes() == b"".join(tm.challenge_cell(c).tobytes() for c in challenges), (name, mode)
        states.append(np.fromfile(d / "state.bin", np.uint8))
        words = tm.state_words(states[-1])
        assert {i: words[i] for i in (8, 25, 26, 27, 28, 29, 30, 31)} == expected_state_words(t, capacity), (name, mode)
    assert states[0].tobytes() == states[1].tobytes(), name


def test_the_overflow_changes_no_challenge_and_the_cases_are_what_they_say():
    cases = tc.cases()
    cut, room = cases["overflow"], cases["overflow_with_room"]
    assert cut.ops == room.ops and cut.capacity % tm.PROOF_ITEM == 16 and room.capacity is None
    t, _ = tm.run(cut.ops)
    assert 0 < cut.capacity < len(t.proof) - tm.PROOF_ITEM and t.status(cut.capacity)["proof_missed"] == len(t.proof) - cut.capacity
    fills = set()
    t = tm.Transcript()
    for name, items in cases["singles"].ops[:-1]:
        fills.add(t.absorbed % tc.BLOCK)
        getattr(t, name)(items)
    assert fills == set(range(tc.BLOCK))  # every offset of a block is where some call began
    for name, first, count in (("identity_first", 0, 1), ("identity_last", 6, 1), ("identity_twice", 2, 3)):
        st = tm.run(cases[name].ops)[0].status()
        assert (st["first_identity"], st["identities"]) == (first, count), name


def test_the_cases_beyond_the_first_chunk_are_what_they_say(drivers):
    chunk_points, chunk_scalars = [int(v) for v in drivers("constants")[0].split()][:2]
    cases = tc.cases(chunk_points, chunk_scalars)
    every = {0} | set(range(1, tc.BLOCK + 1))
    # the two sweeps: every call is a chunk and one item, the model enters them at the fills the arithmetic gives, and between
    # the two every fill is entered, the full block included
    entered = {}
    for name, kind, chunk, message in (("every_fill_into_long_scalars", "write_scalars", chunk_scalars, tm.SCALAR_MESSAGE),
                                       ("every_fill_into_long_points", "write_points", chunk_points, tm.POINT_MESSAGE)):
        ops = cases[name].ops
        calls = [items for op, items in ops if op != "squeeze"]
        assert len(calls) == tc.BLOCK and all(len(items) == chunk + 1 for items in calls) and {op for op, _ in ops} == {kind, "squeeze"}
        assert (chunk + 1) * message % 2 == 1 and ops[-1] == tc.SQUEEZE and sum(op == tc.SQUEEZE for op in ops[1:]) == tc.BLOCK // 16
        entered[name] = {fill for _at, fill in tc.entry_fills(ops)}
        assert entered[name] == tc.sweep_fills(ops, (chunk + 1) * message), name
    assert entered["every_fill_into_long_scalars"] | entered["every_fill_into_long_points"] == every
    assert len({p for _op, items in cases["every_fill_into_long_points"].ops[1:] if items for p in items}) == 256  # the basis, cyclically
    # the longest stream: the long call finds a full block, and its first chunk lays a whole chunk behind it
    for name, chunk, message in (("full_block_then_longest_stream_scalars", chunk_scalars, tm.SCALAR_MESSAGE), ("full_block_then_longest_stream_points", chunk_points, tm.POINT_MESSAGE)):
        ops = cases[name].ops
        (at, fill), = [(at, fill) for at, fill in tc.entry_fills(ops) if len(ops[at][1]) == 2 * chunk + 1]
        assert fill == tc.BLOCK and tc.SQUEEZE not in ops[:at] and ops[at + 1:] == (tc.SQUEEZE,), name
        stream = fill + chunk * message
        assert stream == (128 + 32 * 65 if name.endswith("points") else 128 + 64 * 33), name  # 2240 bytes: the longest the kernel lays out
    # calls that are whole chunks, one and two, of either kind
    sizes = [(op, len(items)) for op, items in cases["exact_chunks"].ops if items]
    assert sizes == [("write_points", chunk_points), ("write_points", 2 * chunk_points), ("write_scalars", chunk_scalars), ("write_scalars", 2 * chunk_scalars)]
    assert [op for op, _items in cases["exact_chunks"].ops[1::2]] == ["squeeze"] * 4
    # the identities
    ops = cases["identity_across_chunks"].ops
    assert ops[0][0] == "common_points" and len(ops[0][1]) == 2 and len(ops[1][1]) == 2 * chunk_points + 3
    assert [i for i, p in enumerate(ops[1][1]) if p is None] == [chunk_points - 1, chunk_points, 2 * chunk_points + 2]
    t = tm.run(ops)[0]
    assert (t.first_identity, t.identities) == (2 + chunk_points - 1, 3)
    assert [i for i in range(len(t.proof) // 32) if t.proof[32 * i:32 * i + 32] == bytes(32)] == [chunk_points - 1, chunk_points, 2 * chunk_points + 2]
    t = tm.run(cases["identity_in_the_second_chunk"].ops)[0]
    assert (t.first_identity, t.identities) == (2 + 2 * chunk_points - 1, 2) and t.first_identity - 2 >= chunk_points
    pts = cases["half_identities"].ops[0][1]
    halves = [(bool(p[0]), bool(p[1])) for p in pts if p is not None]
    assert (False, True) in halves and (True, False) in halves and pts[-1] is None and pts.count(None) == 1
    assert any(a is not None and b is not None and a[1] == 0 and b[0] == 0 and a[0] and b[1] for a, b in zip(pts, pts[1:]))  # y = 0 next to x = 0
    t = tm.run(cases["half_identities"].ops)[0]
    assert (t.first_identity, t.identities) == (len(pts) - 1, 1) and t.proof.count(bytes(32)) == 1 and t.proof.endswith(bytes(32))
    # a proof buffer that ends inside a sixteen-byte piece: 1 and 15 bytes of room in either piece of the third item
    room, model = cases["overflow_with_room"], tm.run(cases["overflow"].ops)[0]
    assert sorted((c - 2 * tm.PROOF_ITEM) // tc.PIECE for c in tc.CUT_INSIDE_A_PIECE) == [0, 0, 1, 1]
    assert sorted(c % tc.PIECE for c in tc.CUT_INSIDE_A_PIECE) == [1, 1, tc.PIECE - 1, tc.PIECE - 1]  # the room in the piece that is cut
    for capacity in tc.CUT_INSIDE_A_PIECE:
        cut = cases["overflow_at_%d" % capacity]
        assert cut.ops == room.ops and cut.capacity == capacity and 2 * tm.PROOF_ITEM < capacity < 3 * tm.PROOF_ITEM
        assert model.status(capacity)["proof_missed"] == len(model.proof) - capacity
