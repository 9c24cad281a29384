"""libaesw_open.so in Python integers (include/aesw_open.h): plain values mod r over tests/ntt_model.py's R, to_cells and
from_cells, every function the serial definition.

  evaluate(coeff, z)          sum coeff[i] z^i, power by power (ntt_model.evaluate is Horner: the two are held equal)
  fold(columns, v, acc)       acc = acc * v + column, column after column, cell by cell
  divide(coeff, z)            (q, rem): S_n = 0, S_i = coeff[i] + z S_(i+1); q[i] = S_(i+1), rem = S_0
  times_linear(q, z, rem)     the coefficients of q(X) (X - z) + rem: what divide must give the column back through

A column of 2^19 cells takes about a second a function."""
from ntt_model import R


def evaluate(coeff, z):
    acc, power = 0, 1
    for c in coeff:
        acc = (acc + c * power) % R
        power = power * z % R
    return acc


def fold(columns, v, acc=None):
    out = list(acc) if acc is not None else [0] * len(columns[0])
    for column in columns:
        out = [(a * v + c) % R for a, c in zip(out, column)]
    return out


def divide(coeff, z):
    n = len(coeff)
    q, s = [0] * n, 0  # s = S_(i+1)
    for i in range(n - 1, -1, -1):
        q[i] = s
        s = (coeff[i] + z * s) % R
    return q, s


def times_linear(q, z, rem):
    """q(X) * (X - z) + rem, len(q) coefficients; q's last coefficient must be 0 for the product to fit"""
    assert q[-1] == 0
    return [((q[i - 1] if i else 0) - z * q[i] + (rem if i == 0 else 0)) % R for i in range(len(q))]
