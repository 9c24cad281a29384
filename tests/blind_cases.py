"""What the tests of libaesw_blind.so share (a helper module, not a test; imports without a GPU): the shapes, the seeds, the special
tail cells with their expected commitments over tests/msm_model.py's basis of known logarithms, and the kernels a GPU sweep
launches.  tests/test_blind_library.py holds every kernel of the library against launched()."""
import functools

import numpy as np

import blind_model as bm
import field_cases as fc
import msm_cases as mc
import msm_model as mm

K = 10
STORE_MODES = (0, 1, 2)  # "fr_store_mode": one instantiation of the fill kernel each
NAMESPACE = "aesw_blind"
COLS = (1, 3)
# the rows of a tail: 65 and 257 pass a wave and a 256-thread workgroup, and n_cols * tail is a multiple of neither; 2^k is every row
FILL_TAILS = (1, 6, 64, 65, 257, 1 << K)
COMMIT_TAILS = (1, 6, 63, 64)
DOMAIN, BIG_DOMAIN, FIRST_COLUMN = 7, (1 << 32) + 5, 3
SEEDS = {"zeros": bytes(32), "ones": b"\xff" * 32, "random": np.random.default_rng(0x626c696e64).bytes(32)}
SEED = SEEDS["random"]


def launched():
    """every __global__ of the library: blind_rows / blinding_tail under the three store modes, commit_tail"""
    return {"%s::blind_cells_kernel<%d>" % (NAMESPACE, m) for m in STORE_MODES} | {"%s::blind_commit_tail_kernel" % NAMESPACE}


def special_cells():
    """raw cells as they lie in memory, from tests/field_cases.py: 0, 1, r - 1, the Montgomery 1 (the cell of the value 1), a lone top limb"""
    return (0, 1, mm.R - 1, fc.FR.one, 1 << 224)


def raw_cells(raws):
    """uint8 [len, 32]: raw limb patterns as cells"""
    return np.frombuffer(b"".join(int(w).to_bytes(32, "little") for w in raws), np.uint8).reshape(len(raws), 32).copy()


@functools.lru_cache(maxsize=None)
def commit_tail_values(tail, n_cols, seed=0x7461696c):
    """[n_cols][tail] plain values: the special cells first (as far as the tail reaches), then seeded scalars"""
    special = [fc.plain(fc.FR, w) for w in special_cells()]
    columns = []
    for j in range(n_cols):
        seeded = mm.seeded_scalars(tail, seed + 64 * j + tail)
        first = special[j:] + special[:j]  # another special cell leads each column
        columns.append(tuple((first + seeded)[:tail]))
    return tuple(columns)


def basis_cells(k):
    return mc.basis_cells(k)


def expected_commit(log, tail, first_row):
    """uint8 [64]: log * G + sum_i tail[i] * P_(first_row + i) over the basis of known logarithms"""
    return mm.to_points([bm.known_commit_tail(log, tail, first_row)])[0]


def cancelling_tail(log, first_row, tail):
    """`tail` plain values whose terms sum to -log * G: seeded ones, and a last one that solves for the rest"""
    values = mm.seeded_scalars(tail - 1, 0x63616e63 + tail)
    rest = (log + sum(v * (mm.E0 + (first_row + i) * mm.D) for i, v in enumerate(values))) % mm.R
    last_log = mm.E0 + (first_row + tail - 1) * mm.D
    return values + [(-rest) * pow(last_log, -1, mm.R) % mm.R]
