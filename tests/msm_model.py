"""bn256's G1 in Python integers, the specification of libaesw_msm.so (a helper module, not a test): y^2 = x^3 + 3 over Fq,
cofactor 1, the group of prime order r.  A point is None (the identity) or (x, y), plain integers below q.  The affine law with
pow(.., -1, q), double-and-add, the naive multi-scalar product, and a second, cheap oracle for any size: a basis whose logarithms
are known, P_i = (e0 + i d) G -- one affine addition a point to build, and sum_i s_i P_i = ((sum_i s_i (e0 + i d)) mod r) G, one
scalar multiplication to expect.  Cells are as they lie in memory: a coordinate is v * 2^256 mod q, little-endian; an affine point
is x then y, 64 bytes, and the identity is 64 zero bytes."""
import functools

import numpy as np

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47  # the base field
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of the group, and of the scalar field
B = 3
GENERATOR = (1, 2)
MONT_Q = (1 << 256) % Q
MONT_Q_INV = pow(MONT_Q, -1, Q)
MONT_R = (1 << 256) % R


def on_curve(p):
    return p is None or (0 <= p[0] < Q and 0 <= p[1] < Q and (p[1] * p[1] - p[0] ** 3 - B) % Q == 0)


def neg(p):
    return None if p is None else (p[0], -p[1] % Q)


def add(p, q):
    """the affine law, every case"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        slope = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        slope = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (slope * slope - p[0] - q[0]) % Q
    return x, (slope * (p[0] - x) - p[1]) % Q


def mul(s, p):
    """s * p by double-and-add, s any integer (reduced mod r)"""
    s %= R
    acc = None
    while s:
        if s & 1:
            acc = add(acc, p)
        p = add(p, p)
        s >>= 1
    return acc


def msm(scalars, points):
    """sum_i scalars[i] * points[i], term by term"""
    acc = None
    for s, p in zip(scalars, points):
        acc = add(acc, mul(s, p))
    return acc


# ---- the basis of known logarithms -------------------------------------------------------------------------------------------------

E0, D = 0x6d736d5f6530, 0x6d736d5f64  # any two values: the logarithm of point i is E0 + i * D


@functools.lru_cache(maxsize=None)
def known_basis(n, e0=E0, d=D):
    """(P_0 ... P_(n-1)), P_i = (e0 + i d) G: one affine addition a point"""
    step = mul(d, GENERATOR)
    points = [mul(e0, GENERATOR)]
    for _ in range(n - 1):
        points.append(add(points[-1], step))
    return tuple(points)


def known_commit(scalars, e0=E0, d=D):
    """sum_i scalars[i] * known_basis[i] by the logarithms: one scalar multiplication"""
    return mul(sum(int(s) * (e0 + i * d) for i, s in enumerate(scalars)) % R, GENERATOR)


# ---- cells -------------------------------------------------------------------------------------------------------------------------

def fq_bytes(v):
    return (v * MONT_Q % Q).to_bytes(32, "little")


def to_points(points):
    """uint8 [len, 64]: affine points in Montgomery form as they lie in memory, the identity as zero bytes"""
    raw = b"".join(bytes(64) if p is None else fq_bytes(p[0]) + fq_bytes(p[1]) for p in points)
    return np.frombuffer(raw, np.uint8).reshape(len(points), 64).copy()


def from_points(cells):
    """the points of uint8 [..., 64] cells; 64 zero bytes are the identity"""
    out = []
    for row in np.ascontiguousarray(cells, np.uint8).reshape(-1, 64):
        x, y = (int.from_bytes(row[i:i + 32].tobytes(), "little") * MONT_Q_INV % Q for i in (0, 32))
        out.append(None if not row.any() else (x, y))
    return out


def canonical_points(points):
    """uint8 [len, 64]: plain little-endian coordinates, what a host reads from a params file"""
    raw = b"".join(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little") for p in points)
    return np.frombuffer(raw, np.uint8).reshape(len(points), 64).copy()


def scalar_cells(values):
    """uint8 [len, 32]: the Montgomery Fr cells of plain scalars"""
    return np.frombuffer(b"".join((int(v) % R * MONT_R % R).to_bytes(32, "little") for v in values), np.uint8).reshape(len(values), 32).copy()


def seeded_scalars(n, seed):
    raw = np.random.default_rng(seed).bytes(40 * n)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % R for i in range(n)]
