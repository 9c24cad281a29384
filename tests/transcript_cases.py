"""What the tests of libaesw_transcript.so share (a helper module, not a test): the op sequences, stated as conditions and found by
search over tests/transcript_model.py, the inputs as they lie in memory, and the kernels a GPU sweep launches.

An op is (name, items): "common_points" / "write_points" with a list of points (None: the identity), "common_scalars" /
"write_scalars" with a list of plain scalars, ("squeeze", None), ("init", None).  A case is its ops and the capacity of the proof
buffer (None: room for everything).  The points are the model's basis of known logarithms, the scalars are seeded."""
import functools
import itertools
from collections import namedtuple

import msm_model as mm
import transcript_model as tm

NAMESPACE = "aesw_transcript"
KERNELS = ("transcript_init_kernel", "transcript_absorb_kernel<true>", "transcript_absorb_kernel<false>", "transcript_squeeze_kernel")
BLOCK = 128
SQUEEZE = ("squeeze", None)
INIT = ("init", None)
PIECE = 16  # the absorb kernel stores the proof sixteen bytes a lane
CUT_INSIDE_A_PIECE = tuple(2 * tm.PROOF_ITEM + piece * PIECE + room for piece in (0, 1) for room in (1, PIECE - 1))
Case = namedtuple("Case", "ops capacity")


def launched():
    """every __global__ of the library: Context.transcript launches init, the points and scalars methods the two absorb kernels,
    squeeze the last"""
    return {"%s::%s" % (NAMESPACE, k) for k in KERNELS}


def points(n, first=0):
    """a fresh list of n points of the basis of known logarithms, from point `first` on"""
    return list(mm.known_basis(256)[first:first + n])


@functools.lru_cache(maxsize=None)
def _scalars(n, seed):
    return tuple(mm.seeded_scalars(n, seed))


def scalars(n, seed=0x7472):
    return list(_scalars(n, seed))


def absorbed_to(length):
    """The shortest run of ops -- a points, then b scalars, then c squeezes, found by search: fewest ops, and of those one that
    holds both kinds -- at whose last squeeze the absorbed length, that squeeze's own 0x00 included, is exactly `length`."""
    best = None
    for a, b in itertools.product(range(length // tm.POINT_MESSAGE + 1), range(length // tm.SCALAR_MESSAGE + 1)):
        c = length - a * tm.POINT_MESSAGE - b * tm.SCALAR_MESSAGE
        key = (a + b + c, not (a and b), c)  # among the shortest, one that holds both kinds
        if c >= 1 and (best is None or key < best[0]):
            best = (key, (a, b, c))
    a, b, c = best[1]
    ops = ([("write_points", points(1, i))] for i in range(a)), ([("common_scalars", scalars(b)[i:i + 1])] for i in range(b)), ([SQUEEZE] for _ in range(c))
    ops = [op for group in ops for run in group for op in run]
    t, _ = tm.run(ops)
    assert t.absorbed == length, (length, a, b, c)
    return ops


def fill_of(t):
    """word 25 of the state a model transcript stands for: 0 when nothing was absorbed, else 1 ... 128 -- a full block stays
    (the lazy last block)"""
    return t.absorbed - (t.absorbed - 1) // BLOCK * BLOCK if t.absorbed else 0


def entry_fills(ops):
    """[(op index, the fill the call finds)] for every absorbing op, on the model"""
    t, out = tm.Transcript(), []
    for i, (name, items) in enumerate(ops):
        if name == "init":
            t = tm.Transcript()
        elif name == "squeeze":
            t.squeeze()
        else:
            out.append((i, fill_of(t)))
            getattr(t, name)(items)
    return out


def filled_block():
    """The fewest items -- a points in one write_points call, then b scalars in one common_scalars call, found by search; of the
    fewest, one that holds both kinds -- after which the block is full and no squeeze has run: the fill is 128."""
    best = None
    for a, b in itertools.product(range(2 * BLOCK), repeat=2):
        if a + b and (a * tm.POINT_MESSAGE + b * tm.SCALAR_MESSAGE) % BLOCK == 0:
            key = (a + b, not (a and b))
            if best is None or key < best[0]:
                best = (key, (a, b))
    a, b = best[1]
    ops = ([("write_points", points(a))] if a else []) + ([("common_scalars", scalars(b, 0x66756c6c))] if b else [])
    assert fill_of(tm.run(ops)[0]) == BLOCK and SQUEEZE not in ops, (a, b)
    return ops


def sweep(name, per_call, take, first=()):
    """`first`, then 128 calls of `name` with per_call items each (take(i): the items of call i), a squeeze behind every 16th"""
    ops = list(first)
    for i in range(BLOCK):
        ops.append((name, take(i)))
        if i % 16 == 15:
            ops.append(SQUEEZE)
    assert sum(1 for op, items in ops if op == name and len(items) == per_call) == BLOCK
    return ops


def sweep_fills(ops, step):
    """The fills the calls of a sweep enter at, by arithmetic alone: a call adds `step` bytes, a squeeze one."""
    absorbed, out = 0, set()
    for name, _items in ops:
        if name == "squeeze":
            absorbed += 1
        else:
            out.add(absorbed - (absorbed - 1) // BLOCK * BLOCK if absorbed else 0)
            absorbed += step
    return out


def _with_identity(at, n=5):
    pts = points(n, 8)
    for i in at:
        pts[i] = None
    return pts


def half_identity_points():
    """What lies in a write_points call whose points are no curve points (the transcript absorbs coordinates and checks no
    equation): (0, y), (x, 0), the adjacent pair (x', 0), (0, y') -- the lanes of that pair's y and of the next point's x are both
    zero -- and one true identity behind them.  Both y are odd, so that the 32 bytes written for (0, y) are not all zero."""
    basis = mm.known_basis(64)
    ys = [p[1] for p in basis if p[1] % 2 == 1][:2]
    xs = [p[0] for p in basis if p[0]][:2]
    pts = [basis[40], (0, ys[0]), (xs[0], 0), (xs[1], 0), (0, ys[1]), None]
    assert all(v for v in xs + ys) and [tm.point_compressed(p) == bytes(32) for p in pts] == [False] * 5 + [True]
    return pts


@functools.lru_cache(maxsize=None)
def cases(chunk_points=32, chunk_scalars=64):
    """name -> Case.  The two chunk sizes are the library's (aesw_transcript_chunk_points / _scalars): the long calls pass two
    chunks and end inside a third.  What a case is for is a condition that tests/test_transcript_model.py asserts on the model."""
    n_points, n_scalars = 4 * chunk_points + 2, 2 * chunk_scalars + 2
    many = scalars(BLOCK, 0x6f6666)
    out = {
        # 33 is odd: over 128 one-scalar calls the block's fill passes every offset mod 128
        "singles": [("write_scalars" if i % 2 else "common_scalars", [many[i]]) for i in range(BLOCK)] + [SQUEEZE],
        "scalars_in_one_call": [("write_scalars", scalars(n_scalars, 0x6f6e65)), SQUEEZE],
        "points_in_one_call": [("write_points", points(n_points)), SQUEEZE],
        "squeeze_first": [SQUEEZE, SQUEEZE, ("write_points", points(1)), SQUEEZE],
        "interleaved": [("common_points", points(1)), ("write_scalars", scalars(2)), SQUEEZE, ("write_points", points(2, 1)), ("common_scalars", scalars(1, 9)), SQUEEZE,
                        ("write_points", points(1, 3)), ("write_scalars", scalars(3, 7)), SQUEEZE],
        "identity_first": [("write_points", _with_identity((0,))), SQUEEZE],
        "identity_last": [("common_points", points(2)), ("write_points", _with_identity((4,))), SQUEEZE],
        "identity_twice": [("write_points", points(1)), ("write_points", _with_identity((1, 3))), SQUEEZE, ("write_points", [None]), SQUEEZE],
        "init_on_a_dirty_state": [("write_points", points(3)), ("write_scalars", scalars(2)), SQUEEZE, INIT, ("write_scalars", scalars(1, 5)), ("write_points", points(2, 5)),
                                  SQUEEZE],
    }
    for length in (BLOCK, 2 * BLOCK):  # the lazy last block: a squeeze that finalises a copy of a full block, and what comes after it
        out["squeeze_at_%d_then_squeeze" % length] = absorbed_to(length) + [SQUEEZE]
        out["squeeze_at_%d_then_absorb" % length] = absorbed_to(length) + [("write_scalars", scalars(1, 3)), SQUEEZE]
    # Calls of a chunk and one item, entered at every fill.  Such a call moves the fill by 65 * 33 = 2145 = 97 (mod 128), which is
    # odd, so 128 of them would pass every residue; a squeeze behind every 16th (a failure then names sixteen calls) moves the
    # rest on by one, and some fills are met twice and some never.  The points sweep starts one byte later than the scalars
    # sweep -- a squeeze first -- and between them every fill is entered: test_transcript_model.py asserts it on the model.
    basis, long_points, long_scalars = mm.known_basis(256), chunk_points + 1, chunk_scalars + 1
    sweep_scalars = scalars(BLOCK * long_scalars, 0x6c6f6e67)
    out["every_fill_into_long_scalars"] = sweep("write_scalars", long_scalars, lambda i: sweep_scalars[i * long_scalars:(i + 1) * long_scalars])
    out["every_fill_into_long_points"] = sweep("write_points", long_points, lambda i: [basis[(i * long_points + j) % len(basis)] for j in range(long_points)], first=[SQUEEZE])
    # the longest stream the absorb kernel holds: a full block kept, and a whole chunk behind it
    out["full_block_then_longest_stream_scalars"] = filled_block() + [("write_scalars", scalars(2 * chunk_scalars + 1, 0x6c73)), SQUEEZE]
    out["full_block_then_longest_stream_points"] = filled_block() + [("write_points", points(2 * chunk_points + 1, 64)), SQUEEZE]
    # calls that are whole chunks: the last turn of the loop is a full one
    out["exact_chunks"] = [("write_points", points(chunk_points, 3)), SQUEEZE, ("write_points", points(2 * chunk_points, 50)), SQUEEZE,
                           ("write_scalars", scalars(chunk_scalars, 0x6578)), SQUEEZE, ("write_scalars", scalars(2 * chunk_scalars, 0x6579)), SQUEEZE]
    # identities at the last item of a chunk, at the first of the next and at the very end, behind two points of an earlier call
    out["identity_across_chunks"] = [("common_points", points(2)), ("write_points", _with_identity((chunk_points - 1, chunk_points, 2 * chunk_points + 2), 2 * chunk_points + 3)),
                                     SQUEEZE]
    # the first identity in a later chunk, at its last item: what the first chunk counts as done enters its index
    out["identity_in_the_second_chunk"] = [("common_points", points(2)), ("write_points", _with_identity((2 * chunk_points - 1, 2 * chunk_points + 2), 2 * chunk_points + 3)), SQUEEZE]
    out["half_identities"] = [("write_points", half_identity_points()), SQUEEZE]
    found = {name: Case(tuple(ops), None) for name, ops in out.items()}
    # a proof buffer that ends in the middle of an item: m = 3 of the 7 items written, the first call fits, the second is cut, the third misses
    overflow = (("write_points", points(2)), ("write_scalars", scalars(3)), SQUEEZE, ("write_points", points(2, 2)), SQUEEZE)
    found["overflow"] = Case(overflow, tm.PROOF_ITEM * 3 - 16)
    found["overflow_with_room"] = Case(overflow, None)
    # cut inside a 16-byte piece: 1 and 15 bytes of room in the first piece of the third item, and in its second
    for capacity in CUT_INSIDE_A_PIECE:
        found["overflow_at_%d" % capacity] = Case(overflow, capacity)
    assert found["identity_twice"].ops[1][1].count(None) == 2
    return found


def item_bytes(name, items):
    """the items of an op as they lie in memory: uint8 [n, 64] points or uint8 [n, 32] cells in Montgomery form"""
    return mm.to_points(items) if name.endswith("points") else mm.scalar_cells(items)


def proof_buffer(ops, capacity, canary):
    """a proof buffer of `capacity` bytes that held `canary` throughout, after the ops: every init moves the cursor back to 0 and
    leaves what was written, so the runs between two inits lie over each other"""
    buf, run = bytearray([canary]) * capacity, []
    for op in list(ops) + [INIT]:
        if op == INIT:
            proof = tm.run(run)[0].proof[:capacity]
            buf[:len(proof)] = proof
            run = []
        else:
            run.append(op)
    return bytes(buf)
