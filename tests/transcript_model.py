"""The Blake2b transcript in Python, the specification of libaesw_transcript.so (a helper module, not a test): halo2's
Blake2bWrite<_, G1Affine, Challenge255<_>> as include/aesw_transcript.h restates it, over hashlib.blake2b -- which keeps the lazy
last block itself -- and the integers of tests/msm_model.py.  A point is None (the identity) or (x, y), plain integers below q; a
scalar is a plain integer.  The identity is absorbed as 0x01 and 64 zero bytes and written as 32 zero bytes, and counted."""
import hashlib

import numpy as np

import msm_model as mm

R, Q = mm.R, mm.Q
PERSON = b"Halo2-Transcript"
STATE_BYTES = 256
POINT_MESSAGE, SCALAR_MESSAGE, PROOF_ITEM = 65, 33, 32


def point_message(p):
    x, y = (0, 0) if p is None else p
    return b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little")


def scalar_message(s):
    return b"\x02" + (s % R).to_bytes(32, "little")


def point_compressed(p):
    x, y = (0, 0) if p is None else p
    return (x | (y & 1) << 255).to_bytes(32, "little")


def scalar_written(s):
    return (s % R).to_bytes(32, "little")


def challenge_of(digest):
    """the 64 bytes as a little-endian integer mod r"""
    return int.from_bytes(digest, "little") % R


def challenge_cell(value):
    """uint8 [32]: the Montgomery cell of a challenge"""
    return mm.scalar_cells([value])[0]


class Transcript:
    """The transcript with an unbounded proof; `absorbed` counts the bytes that went into the hash."""

    def __init__(self):
        self.hash = hashlib.blake2b(digest_size=64, person=PERSON)
        self.proof = b""
        self.absorbed = 0
        self.points = 0
        self.identities = 0
        self.first_identity = None

    def _absorb(self, message):
        self.hash.update(message)
        self.absorbed += len(message)

    def common_points(self, points):
        for p in points:
            if p is None:
                self.identities += 1
                if self.first_identity is None:
                    self.first_identity = self.points
            self.points += 1
            self._absorb(point_message(p))
        return self

    def write_points(self, points):
        self.common_points(points)
        self.proof += b"".join(point_compressed(p) for p in points)
        return self

    def common_scalars(self, scalars):
        for s in scalars:
            self._absorb(scalar_message(s))
        return self

    def write_scalars(self, scalars):
        self.common_scalars(scalars)
        self.proof += b"".join(scalar_written(s) for s in scalars)
        return self

    def squeeze(self):
        self._absorb(b"\x00")
        return challenge_of(self.hash.copy().digest())

    def status(self, capacity=None):
        """the four report words for a proof buffer of `capacity` bytes (None: everything fits)"""
        missed = 0 if capacity is None else max(0, len(self.proof) - capacity)
        return {"proof_bytes": len(self.proof), "proof_missed": missed, "identities": self.identities, "first_identity": self.first_identity}


def run(ops):
    """(the transcript after `ops`, the challenges of its squeezes in order).  An op is (name, items): "common_points",
    "write_points", "common_scalars", "write_scalars" with a list, "squeeze" or "init" with None ("init": a fresh transcript;
    the challenges stay)."""
    t, challenges = Transcript(), []
    for name, items in ops:
        if name == "init":
            t = Transcript()
        elif name == "squeeze":
            challenges.append(t.squeeze())
        else:
            getattr(t, name)(items)
    return t, challenges


def state_words(state):
    """the 32 words of a state as it lies in memory (uint8 [256])"""
    return [int(v) for v in np.ascontiguousarray(state, np.uint8).view("<u8")]
