"""libaesw_shplonk.so in Python integers (include/aesw_shplonk.h): plain values mod r, twice.

  halo2_quotient(columns, evals, pts, y)   Q_i as halo2 writes it: per column R_ij by Lagrange, P_ij - R_ij, the fold under y,
                                           div_by_vanishing as t successive open_model.divide calls with the remainders dropped
  partial_quotient(numer, pts)             (Q_i, remainders) by partial fractions: sum_s w_s kate(N_i, z_s) -- what the device computes
  opening(plan, ...)                       the whole stage by the partial form: every table of the scalars block, h, L', W, the report

A plan here is api.MultiopenPlan's shape: plan.sets = [(point indices, column ids)]; columns[i] are set i's columns as lists of
coefficients, evals[i][j][s] the evaluation of column j of set i at the set's point s.  A column of 2^17 cells takes about a
tenth of a second a division."""
from ntt_model import R

import open_model as om


def inv(a):
    """fr_inv: a^(r - 2), and 0 for 0"""
    return pow(a, R - 2, R)


def lagrange(pts, values):
    """the coefficients, constant first, of the polynomial of degree below len(pts) through (pts[s], values[s]); pts distinct"""
    out = [0] * len(pts)
    for s, (z, e) in enumerate(zip(pts, values)):
        basis, denom = [1], 1
        for r, other in enumerate(pts):
            if r != s:
                basis = [((basis[d - 1] if d else 0) - other * (basis[d] if d < len(basis) else 0)) % R for d in range(len(basis) + 1)]
                denom = denom * (z - other) % R
        scale = e * inv(denom) % R
        out = [(o + scale * b) % R for o, b in zip(out, basis)]
    return out


def minus_low(column, low):
    return [(c - low[i]) % R if i < len(low) else c for i, c in enumerate(column)]


def halo2_quotient(columns, evals, pts, y):
    acc, power = [0] * len(columns[0]), 1
    for column, e in zip(columns, evals):
        diff = minus_low(column, lagrange(pts, e))
        acc = [(a + power * d) % R for a, d in zip(acc, diff)]
        power = power * y % R
    for z in pts:  # div_by_vanishing
        acc, _dropped = om.divide(acc, z)
    return acc


def weights(pts):
    """(w_s, the count of ordered pairs with z_s == z_r)"""
    w, zero = [], 0
    for s, z in enumerate(pts):
        prod = 1
        for r, other in enumerate(pts):
            if r != s:
                prod = prod * (z - other) % R
                zero += (z - other) % R == 0
        w.append(inv(prod))
    return w, zero


def neg_interpolant(pts, ebar, w):
    """-R: R = sum_s ebar_s w_s prod_(r != s) (X - z_r), which is lagrange(pts, ebar) where the points are distinct"""
    out = [0] * len(pts)
    for s in range(len(pts)):
        basis = [1]
        for r, other in enumerate(pts):
            if r != s:
                basis = [((basis[d - 1] if d else 0) - other * (basis[d] if d < len(basis) else 0)) % R for d in range(len(basis) + 1)]
        out = [(o - ebar[s] * w[s] * b) % R for o, b in zip(out, basis)]
    return out


def partial_quotient(numer, pts):
    w, _zero = weights(pts)
    out, rems = [0] * len(numer), []
    for z, weight in zip(pts, w):
        q, rem = om.divide(numer, z)
        out = [(o + weight * c) % R for o, c in zip(out, q)]
        rems.append(rem)
    return out, rems


def combine(columns, coefs, low=(), acc=None):
    out = list(acc) if acc is not None else [0] * len(columns[0])
    for coef, column in zip(coefs, columns):
        out = [(o + coef * c) % R for o, c in zip(out, column)]
    return [(o + low[i]) % R if i < len(low) else o for i, o in enumerate(out)]


def prepare(plan, points, evals, y, v):
    """the tables of the small phase after y and v, per set"""
    sets, zero = [], 0
    for i, (idx, cols) in enumerate(plan.sets):
        pts = [points[p] for p in idx]
        ebar = [sum(pow(y, j, R) * evals[i][j][s] for j in range(len(cols))) % R for s in range(len(pts))]
        w, z = weights(pts)
        zero += z
        sets.append(dict(pts=pts, ebar=ebar, w=w, vw=[pow(v, i, R) * x % R for x in w], neg_r=neg_interpolant(pts, ebar, w)))
    return dict(sets=sets, y_pow=[pow(y, j, R) for j in range(max(len(cols) for _idx, cols in plan.sets))], v_pow=[pow(v, i, R) for i in range(len(plan.sets))],
                zero_differences=zero)


def finish(plan, points, prep, u):
    """the tables of the small phase after u"""
    z = [1] * len(plan.sets)
    for i, (idx, _cols) in enumerate(plan.sets):
        for p, point in enumerate(points):
            if p not in idx:
                z[i] = z[i] * (u - point) % R
    z_t = 1
    for point in points:
        z_t = z_t * (u - point) % R
    z0_inv = inv(z[0])
    l_coef = [z0_inv * prep["v_pow"][i] * z[i] % R for i in range(len(z))] + [-z0_inv * z_t % R]
    r_u = [om.evaluate([-c % R for c in s["neg_r"]], u) for s in prep["sets"]]
    l_const = -sum(c * r for c, r in zip(l_coef, r_u)) % R
    l_low = [-sum(l_coef[i] * s["neg_r"][d] for i, s in enumerate(prep["sets"]) if d < len(s["neg_r"])) % R for d in range(8)]
    l_low[0] = (l_low[0] + l_const) % R
    return dict(z=z, z_t=z_t, z0_inv=z0_inv, l_coef=l_coef, l_const=l_const, l_low=l_low, z0_zero=int(z[0] == 0))


def opening(plan, columns, evals, points, y, v, u_of):
    """The whole stage.  u_of(h) gives u once h is known (the transcript between the two).  Returns a dict: prep, fin, the
    numerators N_i, their remainders, h, L' (line), W, the last remainder and the report."""
    prep = prepare(plan, points, evals, y, v)
    numer, rems, h, bad = [], [], [0] * len(columns[0][0]), []
    for i, s in enumerate(prep["sets"]):
        n_i = combine(columns[i], prep["y_pow"], s["neg_r"])
        q, rem = partial_quotient(n_i, s["pts"])
        h = [(a + prep["v_pow"][i] * c) % R for a, c in zip(h, q)]
        numer.append(n_i)
        rems.append(rem)
        if any(rem):
            bad.append(i)
    u = u_of(h)
    fin = finish(plan, points, prep, u)
    line = combine(numer + [h], fin["l_coef"], fin["l_low"])
    w, last = om.divide(line, u)
    report = dict(bad_sets=len(bad), first_bad_set=bad[0] if bad else None, zero_differences=prep["zero_differences"], z0_zero=fin["z0_zero"], last_remainder=last)
    return dict(prep=prep, fin=fin, numer=numer, rems=rems, h=h, u=u, line=line, w=w, report=report)
