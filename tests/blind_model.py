"""The specification of libaesw_blind.so (a helper module, not a test): a blinding cell as hashlib computes it, and the commitment of
a blinded tail over tests/msm_model.py's G1.

  digest = BLAKE2b-512(key = seed[32], person = PERSON, message = le64(domain) || le64(column) || le64(row))
  cell   = the digest as a little-endian integer mod r, in Montgomery form

A cell is a pure function of (seed, domain, column, row); the randomness is the seed's.  commit_tail is the sum the library adds to a
commitment, tail[i] * P_(first_row + i), term by term or -- over msm_model's basis of known logarithms -- as one scalar multiplication."""
import hashlib

import numpy as np

import msm_model as mm

PERSON = b"aesw-blind-cells"  # csrc/aesw_blind.h: BLIND_PERSON0, BLIND_PERSON1
R = mm.R
MONT_R = mm.MONT_R
MONT_R_INV = pow(MONT_R, -1, R)
MAX_TAIL = 64
assert len(PERSON) == 16


def digest(seed, domain, column, row):
    """the 64 bytes"""
    message = b"".join(int(v).to_bytes(8, "little") for v in (domain, column, row))
    return hashlib.blake2b(message, key=bytes(seed), person=PERSON, digest_size=64).digest()


def value(seed, domain, column, row):
    """the plain value of the cell, below r"""
    return int.from_bytes(digest(seed, domain, column, row), "little") % R


def cell_bytes(v):
    """the 32 bytes of the Montgomery cell of a plain value"""
    return (v % R * MONT_R % R).to_bytes(32, "little")


def tail_values(seed, k, n_cols, first_row, domain, first_column=0):
    """[n_cols][2^k - first_row] plain values: what blind_rows writes from first_row on and blinding_tail writes compactly"""
    return [[value(seed, domain, first_column + j, row) for row in range(first_row, 1 << k)] for j in range(n_cols)]


def tail_cells(seed, k, n_cols, first_row, domain, first_column=0):
    """uint8 [n_cols, 2^k - first_row, 32]"""
    values = tail_values(seed, k, n_cols, first_row, domain, first_column)
    raw = b"".join(cell_bytes(v) for column in values for v in column)
    return np.frombuffer(raw, np.uint8).reshape(n_cols, (1 << k) - first_row, 32).copy()


def plain_of_cells(cells):
    """the plain values of uint8 [..., 32] canonical cells"""
    return [int.from_bytes(row.tobytes(), "little") * MONT_R_INV % R for row in np.ascontiguousarray(cells, np.uint8).reshape(-1, 32)]


def commit_tail(commitment, tail, points):
    """commitment + sum_i tail[i] * points[i]: points are the basis points of the tail's rows, tail plain values"""
    acc = commitment
    for s, p in zip(tail, points):
        acc = mm.add(acc, mm.mul(s, p))
    return acc


def known_commit_tail(commitment_log, tail, first_row, e0=mm.E0, d=mm.D):
    """the same over known_basis, the incoming commitment commitment_log * G: one scalar multiplication"""
    return mm.mul((commitment_log + sum(int(s) * (e0 + (first_row + i) * d) for i, s in enumerate(tail))) % R, mm.GENERATOR)
