"""The segments of libaesw_vanish.so in Python integers (include/aesw_vanish.h), on top of quot_model: plain values mod r.

The fold of the quotient's constraints, acc = acc * y + constraint, cut at constraint boundaries: HEAD, PERM(s) per permutation
set, LOOKUP(s) per column set, then the division.  segment_values() writes the constraints of ONE segment from the cells of its
own columns and from the scalars block -- the values a segment needs that are per proof and not per row -- with no line shared
with csrc/aesw_vanish.h; tests/test_vanish_model.py holds the segments, one behind the other, against quot_model.constraints and
quot_model.fold."""
import ntt_model as nm
import quot_model as qm
import sigma_model as sm

R = nm.R
KINDS = ("head", "perm", "lookup", "divide")
TABLES = ("theta", "beta", "gamma", "y", "y_pow", "theta_pow", "tag", "delta", "beta_delta")  # AESW_VANISH_THETA ...
FIXED_CELLS = 14  # the cells of the block in front of the permutation sets' pairs


def segments(n_sets, chunk_len):
    """(kind, set) in the fold's order"""
    return [("head", 0)] + [("perm", s) for s in range(qm.perm_sets(n_sets, chunk_len))] + [("lookup", s) for s in range(n_sets)] + [("divide", 0)]


def segment_len(kind, n_sets, chunk_len):
    return {"head": 3 + qm.perm_sets(n_sets, chunk_len) - 1, "perm": 1, "lookup": 25, "divide": 0}[kind]


def segment_products(kind, s, n_sets, chunk_len):
    """a segment's share of quot_model.products_per_row: what the row shares is booked to PERM(0) and LOOKUP(0)"""
    sets = sm.sets_of(sm.columns(n_sets), chunk_len)
    if kind == "head":
        return 1 + 2 + 3 + 2 * (len(sets) - 1)
    if kind == "perm":
        return 4 * (sets[s][1] - sets[s][0]) + 2 + (2 if s == 0 else 0)
    return 87 + (5 if s == 0 else 0) if kind == "lookup" else 1


def segment_run_products(kind, s, n_sets, chunk_len):
    """the field products per row a call of the segment runs"""
    sets = sm.sets_of(sm.columns(n_sets), chunk_len)
    if kind == "perm":
        return 2 + 4 * (sets[s][1] - sets[s][0]) - 1 + 2
    return 90 if kind == "lookup" else segment_products(kind, s, n_sets, chunk_len)


def products_per_row(n_sets, chunk_len):
    return sum(segment_products(kind, s, n_sets, chunk_len) for kind, s in segments(n_sets, chunk_len))


def scalars(n_sets, chunk_len, theta, beta, gamma, y):
    """table name -> the residues of its entries"""
    firsts = [first for first, _end in sm.sets_of(sm.columns(n_sets), chunk_len)]
    return {"theta": [theta], "beta": [beta], "gamma": [gamma], "y": [y],
            "y_pow": [pow(y, segment_len(kind, n_sets, chunk_len), R) for kind in KINDS[:3]],
            "theta_pow": [pow(theta, 2, R), pow(theta, 3, R)],
            "tag": [t * pow(theta, qm.ARITY[t] - 1, R) % R for t in range(1, 6)],
            "delta": [pow(sm.DELTA, first, R) for first in firsts],
            "beta_delta": [beta * pow(sm.DELTA, first, R) % R for first in firsts]}


def scalars_block(n_sets, chunk_len, theta, beta, gamma, y):
    """the residues of d_scalars in its order: delta^first(s) and beta * delta^first(s) side by side, set by set"""
    sc = scalars(n_sets, chunk_len, theta, beta, gamma, y)
    flat = [v for name in TABLES[:7] for v in sc[name]]
    assert len(flat) == FIXED_CELLS
    return flat + [v for pair in zip(sc["delta"], sc["beta_delta"]) for v in pair]


def offset(table, index):
    """the byte offset of an entry, or None"""
    sizes = {"theta": 1, "beta": 1, "gamma": 1, "y": 1, "y_pow": 3, "theta_pow": 2, "tag": 5}
    if table in sizes:
        return 32 * (sum(sizes[t] for t in TABLES[:TABLES.index(table)]) + index) if index < sizes[table] else None
    return 32 * (FIXED_CELLS + 2 * index + (table == "beta_delta")) if index < sm.columns(1024) else None


def segment_values(kind, s, n_sets, chunk_len, n_rows, x, at, sc):
    """The constraints of one segment in their order at the point x.  at(group, column, r) as quot_model.constraints takes it;
    sc: what scalars() returns."""
    sets = sm.sets_of(sm.columns(n_sets), chunk_len)
    beta, gamma, theta = sc["beta"][0], sc["gamma"][0], sc["theta"][0]
    l0, l_last, l_active = (at("l", i, 0) for i in range(3))
    if kind == "head":
        z_last = at("zperm", len(sets) - 1, 0)
        out = [at("rcon", 1, 0) * (at("advice", 3 * n_sets, 0) - at("rcon", 0, 0)), l0 * (1 - at("zperm", 0, 0)), l_last * (z_last * z_last - z_last)]
        out += [l0 * (at("zperm", i, 0) - at("zperm", i - 1, n_rows)) for i in range(1, len(sets))]
    elif kind == "perm":
        first, end = sets[s]
        sources = sm.sources(n_sets)
        left, right, bx = at("zperm", s, 1), at("zperm", s, 0), sc["beta_delta"][s] * x % R
        for c in range(first, end):
            v = at("advice", sources[c], 0) if sources[c] <= 3 * n_sets else at("rcon", 0, 0)
            left = left * (v + gamma + beta * at("sigma", c, 0)) % R
            right = right * (v + gamma + bx) % R
            bx = bx * sm.DELTA % R
        out = [l_active * (left - right)]
    elif kind == "lookup":
        under = {2: lambda e: (e[0] * theta + e[1]) % R, 3: lambda e: ((e[0] * theta + e[1]) * theta + e[2]) % R,
                 4: lambda e: (((e[0] * theta + e[1]) * theta + e[2]) * theta + e[3]) % R}
        table = [at("table", e, 0) for e in range(4)]
        xyz = [at("advice", 3 * s + e, 0) for e in range(3)]
        out = []
        for t in range(1, 6):
            i, a = 5 * s + t - 1, qm.ARITY[t]
            # q * compress(t, x, y, z) with the tag's term from the block: t * theta^(a - 1) + (x, y, z under the arity)
            inp = at("selectors", i, 0) * (sc["tag"][t - 1] + qm.compress(theta, xyz[:a - 1])) % R
            z, ap, sp = at("zlookup", i, 0), at("a", i, 0), at("s", i, 0)
            out += [l0 * (1 - z), l_last * (z * z - z), l_active * (at("zlookup", i, 1) * (ap + beta) * (sp + gamma) - z * (inp + beta) * (under[a](table) + gamma)),
                    l0 * (ap - sp), l_active * (ap - sp) * (ap - at("a", i, -1))]
    else:
        out = []
    return [c % R for c in out]


def run_segment(kind, s, k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, j, cell, sc, acc_in=0):
    """acc_out at row j of one segment call: the fold from acc_in, or for the division acc_in * inv(x_j^n - 1)"""
    if kind == "divide":
        return acc_in * qm.vanish_inverses(k, ext_k, zeta_sel)[j % (1 << (ext_k - k))] % R
    acc = acc_in
    for v in segment_values(kind, s, n_sets, chunk_len, n_rows, qm.point(ext_k, zeta_sel, j), lambda g, c, r: cell(g, c, qm.rot(k, ext_k, j, r)), sc):
        acc = (acc * sc["y"][0] + v) % R
    return acc


def quotient(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, columns, theta, beta, gamma, y, rows=None):
    """quot_model.quotient segment by segment"""
    sc = scalars(n_sets, chunk_len, theta, beta, gamma, y)
    out = []
    for j in (range(1 << ext_k) if rows is None else rows):
        acc = 0
        for kind, s in segments(n_sets, chunk_len):
            acc = run_segment(kind, s, k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, j, lambda g, c, r: columns[g][c][r], sc, acc)
        out.append(acc)
    return out
