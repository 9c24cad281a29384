"""What the tests of libaesw_msm.so share (a helper module, not a test): the shapes, the scalar columns with their expected
commitments against the basis of known logarithms, the special bases, and the kernels a GPU sweep launches.  The basis is built
once per k by tests/msm_model.py (one affine addition a point) and every expectation is one scalar multiplication, so a shape
costs the model milliseconds."""
import functools

import numpy as np

import msm_model as mm

FR, BYTES = 0, 1
KS = (10, 11)
COLS = (1, 3)
SLICES = (0, 1, 2, 3)  # 3: an uneven last slice
NAMESPACE = "aesw_msm"
KERNELS = ("msm_report_reset_kernel", "msm_basis_kernel", "msm_digits_kernel", "msm_bucket_kernel", "msm_reduce_kernel", "msm_combine_kernel")


def launched():
    """every __global__ of the library: the GPU tests launch each (msm_basis: the first two; commit_columns of cells: the rest)"""
    return {"%s::%s" % (NAMESPACE, k) for k in KERNELS}


@functools.lru_cache(maxsize=None)
def basis_cells(k):
    """uint8 [2^k, 64]: the basis of known logarithms in Montgomery form"""
    return mm.to_points(mm.known_basis(1 << k))


@functools.lru_cache(maxsize=None)
def fr_columns(k):
    """name -> the plain scalars of a column of 2^k cells"""
    n = 1 << k
    same = mm.seeded_scalars(1, 0x73616d65 + k)[0]
    return {
        "seeded": tuple(mm.seeded_scalars(n, 0x6d73 + k)),
        "zero": (0,) * n,
        "one": (1,) * n,
        "r-1": (mm.R - 1,) * n,
        "same": (same,) * n,  # every row in one bucket per window: right, only slow
        "ends": (mm.seeded_scalars(1, 1)[0],) + (0,) * (n - 2) + (mm.seeded_scalars(1, 2)[0],),
        "seeded2": tuple(mm.seeded_scalars(n, 0x6d74 + k)),
    }


@functools.lru_cache(maxsize=None)
def byte_columns(k):
    """name -> the values of a column of 2^k bytes"""
    n = 1 << k
    rng = np.random.default_rng(0x6279 + k)
    return {
        "seeded": tuple(int(v) for v in rng.integers(0, 256, n)),
        "zero": (0,) * n,
        "one": (1,) * n,
        "255": (255,) * n,
        "same": (0x5a,) * n,
        "ends": (7,) + (0,) * (n - 2) + (201,),
        "seeded2": tuple(int(v) for v in rng.integers(0, 256, n)),
    }


def columns(kind, k):
    return fr_columns(k) if kind == FR else byte_columns(k)


def scalar_bytes(kind, values):
    """a column as it lies in memory: uint8 [2^k, 32] cells or uint8 [2^k] bytes"""
    return mm.scalar_cells(values) if kind == FR else np.array(values, np.uint8)


@functools.lru_cache(maxsize=None)
def expected(kind, k, name):
    """uint8 [64]: the commitment of the named column against basis_cells(k), by the logarithms"""
    return mm.to_points([mm.known_commit(columns(kind, k)[name])])[0]


def groups(kind, k, n_cols):
    """the named columns in groups of n_cols, the last group filled up from the front"""
    names = sorted(columns(kind, k))
    return [(names[i:i + n_cols] + names)[:n_cols] for i in range(0, len(names), n_cols)]


def kind_name(kind):
    return "fr" if kind == FR else "bytes"
