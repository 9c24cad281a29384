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


def _with_identity(at):
    pts = points(5, 8)
    for i in at:
        pts[i] = None
    return pts


@functools.lru_cache(maxsize=None)
def cases(chunk_points=32, chunk_scalars=64):
    """name -> Case.  The two chunk sizes are the library's (aesw_transcript_chunk_points / _scalars): the long calls pass two
    chunks and end inside a third."""
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
    found = {name: Case(tuple(ops), None) for name, ops in out.items()}
    # a proof buffer that ends in the middle of an item: m = 3 of the 7 items written, the first call fits, the second is cut, the third misses
    overflow = (("write_points", points(2)), ("write_scalars", scalars(3)), SQUEEZE, ("write_points", points(2, 2)), SQUEEZE)
    found["overflow"] = Case(overflow, tm.PROOF_ITEM * 3 - 16)
    found["overflow_with_room"] = Case(overflow, None)
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
