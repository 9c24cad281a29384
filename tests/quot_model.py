"""The quotient of libaesw_quot.so in Python integers (include/aesw_quot.h), on top of ntt_model and sigma_model: plain values mod r.

numerator() evaluates the folded constraints at ONE row of the extended domain from the cells of that row and of its rotations,
every constraint written out as the header states it -- each lookup input compressed expression by expression, no shared
sub-expression -- and with no line shared with csrc/aesw_quot.h.  tests/test_quot_model.py holds it against the definition: the
columns' polynomials evaluated at the coset points by Horner."""
import numpy as np

import ntt_model as nm
import sigma_model as sm

R = nm.R
GROUPS = ("advice", "rcon", "selectors", "table", "sigma", "zperm", "a", "s", "zlookup", "l")
ARITY = {1: 2, 2: 4, 3: 3, 4: 3, 5: 3}  # theta_arity(theta_table_of_tag(t))


def perm_sets(n_sets, chunk_len):
    return -(-sm.columns(n_sets) // chunk_len)


def group_columns(n_sets, chunk_len):
    """group -> the number of its columns, in the order of the evaluate call"""
    return {"advice": 3 * n_sets + 1, "rcon": 2, "selectors": 5 * n_sets, "table": 4, "sigma": sm.columns(n_sets), "zperm": perm_sets(n_sets, chunk_len),
            "a": 5 * n_sets, "s": 5 * n_sets, "zlookup": 5 * n_sets, "l": 3}


def rot(k, ext_k, j, r):
    return (j + r * (1 << (ext_k - k))) % (1 << ext_k)


def point(ext_k, zeta_sel, j):
    return nm.ZETAS[zeta_sel] * pow(nm.omega(ext_k), j, R) % R


def vanish_inverses(k, ext_k, zeta_sel):
    """inv(x_j^n - 1) by j mod m"""
    return [pow(pow(point(ext_k, zeta_sel, i), 1 << k, R) - 1, -1, R) for i in range(1 << (ext_k - k))]


def tables(k, ext_k, zeta_sel):
    """The residues of d_tables in its order: the m inverses, omega_ext^j, zeta * omega_ext^(j * 2^14)."""
    w = nm.omega(ext_k)
    return vanish_inverses(k, ext_k, zeta_sel) + [pow(w, j, R) for j in range(1 << min(ext_k, 14))] + \
        [nm.ZETAS[zeta_sel] * pow(w, j << 14, R) % R for j in range(1 << max(ext_k - 14, 0))]


def products_per_row(n_sets, chunk_len):
    c, s = sm.columns(n_sets), perm_sets(n_sets, chunk_len)
    return 12 + 4 * s + 4 * c + 87 * n_sets


def compress(theta, expressions):
    acc = 0
    for e in expressions:
        acc = (acc * theta + e) % R
    return acc


def constraints(k, ext_k, n_sets, chunk_len, n_rows, x, at, theta, beta, gamma):
    """The constraints in their order at the point x.  at(group, column, r): that column's polynomial at x * omega^r (the cell of
    the extended column at the row rotated by r)."""
    sets = sm.sets_of(sm.columns(n_sets), chunk_len)
    sources = sm.sources(n_sets)
    l0, l_last, l_active = (at("l", i, 0) for i in range(3))
    out = [at("rcon", 1, 0) * (at("advice", 3 * n_sets, 0) - at("rcon", 0, 0))]
    out.append(l0 * (1 - at("zperm", 0, 0)))
    last = at("zperm", len(sets) - 1, 0)
    out.append(l_last * (last * last - last))
    for s in range(1, len(sets)):
        out.append(l0 * (at("zperm", s, 0) - at("zperm", s - 1, n_rows)))
    for s, (first, end) in enumerate(sets):
        left, right = at("zperm", s, 1), at("zperm", s, 0)
        for c in range(first, end):
            v = at("advice", sources[c], 0) if sources[c] <= 3 * n_sets else at("rcon", 0, 0)
            left = left * (v + beta * at("sigma", c, 0) + gamma) % R
            right = right * (v + beta * pow(sm.DELTA, c, R) * x + gamma) % R
        out.append(l_active * (left - right))
    for s in range(n_sets):
        for t in range(1, 6):
            i = 5 * s + t - 1
            q = at("selectors", i, 0)
            a = ARITY[t]
            inp = compress(theta, [q * t, q * at("advice", 3 * s, 0), q * at("advice", 3 * s + 1, 0), q * at("advice", 3 * s + 2, 0)][:a])
            tab = compress(theta, [at("table", e, 0) for e in range(a)])
            z, ap, sp = at("zlookup", i, 0), at("a", i, 0), at("s", i, 0)
            out.append(l0 * (1 - z))
            out.append(l_last * (z * z - z))
            out.append(l_active * (at("zlookup", i, 1) * (ap + beta) * (sp + gamma) - z * (inp + beta) * (tab + gamma)))
            out.append(l0 * (ap - sp))
            out.append(l_active * (ap - sp) * (ap - at("a", i, -1)))
    return [c % R for c in out]


def fold(values, y):
    acc = 0
    for v in values:
        acc = (acc * y + v) % R
    return acc


def numerator(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, j, cell, theta, beta, gamma, y):
    """cell(group, column, row): the value of that extended column at that row"""
    return fold(constraints(k, ext_k, n_sets, chunk_len, n_rows, point(ext_k, zeta_sel, j), lambda g, c, r: cell(g, c, rot(k, ext_k, j, r)), theta, beta, gamma), y)


def quotient(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, columns, theta, beta, gamma, y, rows=None):
    """out[j] for the rows asked for (default: all): columns a dict group -> list of columns of 2^ext_k values"""
    inverses = vanish_inverses(k, ext_k, zeta_sel)
    m = 1 << (ext_k - k)
    return [numerator(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, j, lambda g, c, r: columns[g][c][r], theta, beta, gamma, y) * inverses[j % m] % R
            for j in (range(1 << ext_k) if rows is None else rows)]


def seeded_columns(ext_k, n_sets, chunk_len, seed):
    """group -> uint8 [count, 2^ext_k, 32] canonical random cells, and the same as values"""
    cells, values = {}, {}
    for i, (g, count) in enumerate(group_columns(n_sets, chunk_len).items()):
        flat = nm.seeded_values(count << ext_k, seed + i)
        values[g] = [flat[c << ext_k:(c + 1) << ext_k] for c in range(count)]
        cells[g] = nm.to_cells(flat).reshape(count, 1 << ext_k, 32)
    return cells, values


def unit_columns(k, n_rows):
    """l0, l_last, l_active as Lagrange columns of 2^k values"""
    n = 1 << k
    return [[int(i == 0) for i in range(n)], [int(i == n_rows) for i in range(n)], [int(i < n_rows) for i in range(n)]]


def cells_of(groups):
    return np.concatenate([groups[g].reshape(-1, 32) for g in GROUPS])
