"""The transforms of libaesw_ntt.so in Python integers (include/aesw_ntt.h): plain values mod r, no Montgomery form.

ntt() is an iterative radix-2 transform (0.6 s for a column of 2^16 rows, 3 s for 2^18, so full-column comparisons stop at k = 18);
tests/test_ntt_model.py holds it against the definition, sum a_i x^i by Horner at every point, for k <= 8.  evaluate() is that
Horner sum, for sampled checks of columns no model run reaches."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of bn256's scalar field
G = 7
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)
ZETAS = (pow(G, (R - 1) // 3, R), pow(G, 2 * (R - 1) // 3, R))  # zeta_sel 0, and its square
assert (R - 1) % 3 == 0 and ZETAS[1] == ZETAS[0] * ZETAS[0] % R and all(pow(z, 3, R) == 1 and z != 1 for z in ZETAS)


def omega(k):
    return pow(G, (R - 1) >> k, R)


def ntt(values, root):
    """[sum_i values[i] * root^(i j) for j], len(values) = 2^k and root of that order: bit-reversed copy, then k stages in place"""
    n = len(values)
    k = n.bit_length() - 1
    assert n == 1 << k
    a = [values[int(format(i, "0%db" % k)[::-1], 2)] if k else values[i] for i in range(n)]
    half = 1
    while half < n:
        step = pow(root, n // (2 * half), R)
        tw = [1] * half
        for i in range(1, half):
            tw[i] = tw[i - 1] * step % R
        for start in range(0, n, 2 * half):
            for i in range(half):
                x, y = a[start + i], a[start + i + half] * tw[i] % R
                a[start + i], a[start + i + half] = (x + y) % R, (x - y) % R
        half *= 2
    return a


def evaluate(coeff, x):
    """sum coeff[i] x^i by Horner"""
    acc = 0
    for c in reversed(coeff):
        acc = (acc * x + c) % R
    return acc


def coeff_to_lagrange(coeff, k):
    return ntt(coeff, omega(k))


def lagrange_to_coeff(values, k):
    scale = pow(1 << k, -1, R)
    return [v * scale % R for v in ntt(values, pow(omega(k), -1, R))]


def coeff_to_extended(coeff, k, ext_k, zeta_sel):
    z = ZETAS[zeta_sel]
    cycle = (1, z, z * z % R)
    return ntt([c * cycle[i % 3] % R for i, c in enumerate(coeff)] + [0] * ((1 << ext_k) - (1 << k)), omega(ext_k))


def extended_to_coeff(values, ext_k, zeta_sel):
    z = pow(ZETAS[zeta_sel], -1, R)
    cycle = (1, z, z * z % R)
    return [c * cycle[i % 3] % R for i, c in enumerate(lagrange_to_coeff(values, ext_k))]


# ---- cells -----------------------------------------------------------------------------------------------------------------------

def to_cells(values):
    """uint8 [len, 32]: the Montgomery cells of plain values, as they lie in memory"""
    return np.frombuffer(b"".join((v * MONT % R).to_bytes(32, "little") for v in values), np.uint8).reshape(len(values), 32).copy()


def from_cells(cells):
    """the plain values of uint8 [..., 32] Montgomery cells (canonical or not: the bytes are reduced)"""
    flat = np.ascontiguousarray(cells, np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") * MONT_INV % R for row in flat]


def seeded_values(n, seed):
    raw = np.random.default_rng(seed).bytes(40 * n)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % R for i in range(n)]
