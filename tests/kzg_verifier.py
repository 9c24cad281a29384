"""The other party of the proof stage in Python integers (a helper module, not a test): a KZG verifier without pairings.

Commit against a basis P_i = tau^i G whose tau the test knows.  Then commit(f) = f(tau) G, and the pairing check of an opening,
e(W, [tau]_2) = e(u W + L, [1]_2), is the group equation (tau - u) W == L, which tests/msm_model.py's affine law decides in a few
scalar multiplications.  What stands here is written from the verifier's side of the SHPLONK paper (Boneh, Drake, Fisch, Gabizon
2020, section 4) and knows none of the prover's tables: it imports the group (msm_model), the field's R and omega (ntt_model) and
the transcript (transcript_model), and neither shplonk_model nor open_model nor any header of the product -- that is its point,
and tests/test_kzg_verifier.py holds it.

  fixed_mul(s)                     s G through a table of the 32 x 255 byte multiples of G: at most 32 affine additions
  tau_basis(k, tau)                (tau^i G), 2^k points;  lagrange_basis(k, tau): (L_i(tau) G) for the rows omega_k^i
  commit(coeff, tau)               f(tau) G by the exponent: one Horner sum and one fixed_mul
  msm(terms)                       sum of s * P with the doublings shared: what keeps a set of 257 columns at a second
  verify_single(C, x, e, Wq, tau)  (tau - x) Wq == C - e G
  verify_shplonk(...)              a Verdict: accepted, or refused with a named reason -- never a division by zero
  read_proof(proof, layout)        the verifier's side of the transcript: the points, the scalars and the challenges of the bytes

A point is None (the identity) or (x, y), as in msm_model."""
import functools

import msm_model as mm
import ntt_model as nm
import transcript_model as tm

R, Q, G1 = nm.R, mm.Q, mm.GENERATOR
assert R == mm.R and Q % 4 == 3
TAU = nm.seeded_values(1, 0x6b7a6774)[0]  # "kzgt": any value that is no row of a domain in use
KS = (10,)
assert all(pow(TAU, 1 << k, R) != 1 for k in KS), "tau must be no 2^k-th root of unity: it would be a row of the domain"


@functools.lru_cache(maxsize=None)
def byte_table():
    """table[w][d - 1] = d * 256^w * G, d = 1 ... 255: 32 x 255 affine additions"""
    table, base = [], G1
    for _w in range(32):
        row = [base]
        for _d in range(254):
            row.append(mm.add(row[-1], base))
        table.append(tuple(row))
        base = mm.add(row[-1], base)  # 256 * base
    return tuple(table)


def fixed_mul(s):
    """(s mod r) G"""
    acc, table = None, byte_table()
    for w, byte in enumerate((s % R).to_bytes(32, "little")):
        if byte:
            acc = mm.add(acc, table[w][byte - 1])
    return acc


@functools.lru_cache(maxsize=None)
def tau_basis(k, tau=TAU):
    out, power = [], 1
    for _ in range(1 << k):
        out.append(fixed_mul(power))
        power = power * tau % R
    return tuple(out)


def lagrange_at(k, tau):
    """[L_i(tau)] for the rows omega_k^i: (tau^n - 1) omega^i / (n (tau - omega^i)); tau on no row"""
    n, omega = 1 << k, nm.omega(k)
    top = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    assert top, "tau is a row of the domain"
    out, row = [], 1
    for _ in range(n):
        out.append(top * row % R * pow(tau - row, -1, R) % R)
        row = row * omega % R
    return out


@functools.lru_cache(maxsize=None)
def lagrange_basis(k, tau=TAU):
    return tuple(fixed_mul(c) for c in lagrange_at(k, tau))


def evaluate(coeff, x):
    acc = 0
    for c in reversed(coeff):
        acc = (acc * x + c) % R
    return acc


def commit(coeff, tau=TAU):
    """what sum_i coeff[i] * tau_basis[i] is, by the exponent"""
    return fixed_mul(evaluate(coeff, tau))


def sub(p, q):
    return mm.add(p, mm.neg(q))


def msm(terms):
    """sum of s * P over (s, P) pairs by msm_model's affine law, the doublings shared: bit by bit from the top"""
    terms = [(s % R, P) for s, P in terms if P is not None and s % R]
    acc = None
    for bit in range(max((s.bit_length() for s, _P in terms), default=0) - 1, -1, -1):
        acc = mm.add(acc, acc)
        for s, P in terms:
            if s >> bit & 1:
                acc = mm.add(acc, P)
    return acc


def verify_single(C, x, e, Wq, tau=TAU):
    """one KZG opening: C opens to e at x with the witness Wq"""
    return mm.mul((tau - x) % R, Wq) == sub(C, fixed_mul(e))


class Verdict:
    """What verify_shplonk returns: true when accepted, else `reason` names why not"""
    REASONS = ("shape", "repeated_point", "z0_zero", "equation")

    def __init__(self, reason=None):
        assert reason is None or reason in self.REASONS
        self.accepted, self.reason = reason is None, reason

    def __bool__(self):
        return self.accepted

    def __repr__(self):
        return "Verdict(accepted)" if self.accepted else "Verdict(refused: %s)" % self.reason


def interpolant_at(pts, values, u):
    """the polynomial of degree below len(pts) through (pts[s], values[s]) at u, term by term; pts distinct"""
    total = 0
    for s, (z, e) in enumerate(zip(pts, values)):
        num = den = 1
        for r, other in enumerate(pts):
            if r != s:
                num, den = num * (u - other) % R, den * (z - other) % R
        total = (total + e * num % R * pow(den, -1, R)) % R
    return total


def verify_shplonk(plan, commitments, evals, points, y, v, u, H, W, tau=TAU):
    """The verifier of SHPLONK's multi-opening.  plan.sets = [(indices into points, column ids)]; commitments[i][j] the point of
    column j of set i, evals[i][j][s] its claimed evaluation at the set's point s; points the super set; y, v, u the challenges;
    H, W the prover's two points.  With e_is = sum_j y^j e_ijs, r_i the interpolant through (z_s, e_is), z_i = prod over the
    points outside set i of (u - p) and z_T = prod over all of them:
        L = sum_i v^i (z_i / z_0) (sum_j y^j C_ij - r_i(u) G) - (z_T / z_0) H,     accept iff (tau - u) W == L."""
    if len(commitments) != len(plan.sets) or len(evals) != len(plan.sets):
        return Verdict("shape")
    for (idx, cols), of_set, e_set in zip(plan.sets, commitments, evals):
        if len(of_set) != len(cols) or len(e_set) != len(cols) or any(len(e) != len(idx) for e in e_set) or any(not 0 <= p < len(points) for p in idx):
            return Verdict("shape")
        if len({points[p] % R for p in idx}) != len(idx):
            return Verdict("repeated_point")  # no interpolant through two values at one point
    z = []
    for idx, _cols in plan.sets:
        prod = 1
        for p, point in enumerate(points):
            if p not in idx:
                prod = prod * (u - point) % R
        z.append(prod)
    if z[0] == 0:
        return Verdict("z0_zero")  # u is a super-set point outside set 0: the normalisation does not exist
    z_t = 1
    for point in points:
        z_t = z_t * (u - point) % R
    z0_inv = pow(z[0], -1, R)
    terms, constant, v_pow = [(-z_t * z0_inv % R, H)], 0, 1  # L as one sum of scalar * point, and the multiple of G apart
    for i, (idx, _cols) in enumerate(plan.sets):
        pts, scale = [points[p] for p in idx], v_pow * z[i] % R * z0_inv % R
        e_bar, y_pow = [0] * len(pts), 1
        for C, e in zip(commitments[i], evals[i]):
            terms.append((scale * y_pow % R, C))
            e_bar = [(a + y_pow * b) % R for a, b in zip(e_bar, e)]
            y_pow = y_pow * y % R
        constant = (constant - scale * interpolant_at(pts, e_bar, u)) % R
        v_pow = v_pow * v % R
    line = mm.add(msm(terms), fixed_mul(constant))
    return Verdict(None if mm.mul((tau - u) % R, W) == line else "equation")


# ---- the transcript, read -------------------------------------------------------------------------------------------------------------

def decompress(raw):
    """the point of 32 proof bytes: x with the parity of y in the top bit, 32 zero bytes the identity (transcript_model.point_compressed)"""
    word = int.from_bytes(raw, "little")
    if word == 0:
        return None
    x, odd = word & ((1 << 255) - 1), word >> 255
    rhs = (x * x * x + mm.B) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    if x >= Q or y * y % Q != rhs:
        raise ValueError("the bytes are no point of the curve")
    return x, (y if y & 1 == odd else Q - y)


def rotated(x, k, rotations):
    """x omega_k^r for every signed rotation r: the points a column is opened at"""
    return [x * pow(nm.omega(k), r % (1 << k), R) % R for r in rotations]


def read_proof(proof, layout):
    """The proof bytes through a fresh transcript in the order the prover wrote them.  layout: a list of ("points", count),
    ("scalars", count) and ("squeeze", name).  Returns (points, scalars, challenges): the parsed points and scalars in order, and
    name -> challenge.  Bytes that are no point, a scalar not below r, and bytes missing or left over raise ValueError."""
    t, at = tm.Transcript(), 0
    points, scalars, challenges = [], [], {}
    for what, arg in layout:
        if what == "squeeze":
            challenges[arg] = t.squeeze()
            continue
        if at + 32 * arg > len(proof):
            raise ValueError("the proof ends at byte %d, inside its %s" % (len(proof), what))
        items = [proof[at + 32 * i:at + 32 * i + 32] for i in range(arg)]
        at += 32 * arg
        if what == "points":
            items = [decompress(raw) for raw in items]
            t.common_points(items)
            points += items
        elif what == "scalars":
            items = [int.from_bytes(raw, "little") for raw in items]
            if any(s >= R for s in items):
                raise ValueError("a scalar of the proof is not below r")
            t.common_scalars(items)
            scalars += items
        else:
            raise ValueError("no such item: %r" % (what,))
    if at != len(proof):
        raise ValueError("%d bytes of the proof are left over" % (len(proof) - at))
    return points, scalars, challenges


def stage_layout(plan):
    """the proof of an opening stage as the tests write it: every column's commitment in the plan's order, x, every evaluation in
    the plan's order, y, v, [h], u, [W]"""
    n_cols, n_evals = sum(len(cols) for _idx, cols in plan.sets), sum(len(idx) * len(cols) for idx, cols in plan.sets)
    return [("points", n_cols), ("squeeze", "x"), ("scalars", n_evals), ("squeeze", "y"), ("squeeze", "v"), ("points", 1), ("squeeze", "u"), ("points", 1)]


def verify_proof(proof, plan, k, tau=TAU):
    """(verdict, what was read): the bytes of stage_layout(plan), the plan (its rotations name the points) and nothing else"""
    points, scalars, ch = read_proof(proof, stage_layout(plan))
    commitments, evals = by_plan(plan, points[:-2], scalars)
    verdict = verify_shplonk(plan, commitments, evals, rotated(ch["x"], k, plan.rotations), ch["y"], ch["v"], ch["u"], points[-2], points[-1], tau)
    return verdict, dict(points=points, scalars=scalars, challenges=ch)


def by_plan(plan, flat_points, flat_evals):
    """commitments[i][j] and evals[i][j][s] from the flat order of the proof: the columns set by set, the evaluations set by set,
    column by column, point by point"""
    commitments, evals, c, e = [], [], 0, 0
    for idx, cols in plan.sets:
        commitments.append(list(flat_points[c:c + len(cols)]))
        c += len(cols)
        evals.append([list(flat_evals[e + j * len(idx):e + (j + 1) * len(idx)]) for j in range(len(cols))])
        e += len(cols) * len(idx)
    assert c == len(flat_points) and e == len(flat_evals)
    return commitments, evals
