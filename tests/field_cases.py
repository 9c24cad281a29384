"""The operand values of tests/test_field_cases.py and tests/test_gpu_field_operands.py (a helper module, not a test): for each of
bn256's fields the 64 raw limb patterns at which carries and borrows run, on top of tests/test_field_headers.py's fields and
CARRIES, and the layouts that bring every ordered pair of them to a product, a sum and a difference of the device.

A raw value is a cell as it lies in memory, eight little-endian limbs, canonical.  The calls of the prover-side libraries take
cells as they lie, so the device arithmetic sees exactly the limbs chosen here; the Python models take plain values, and the raw
pattern w is the cell of plain(field, w) = w / 2^256 mod m, so model(plain(w)) put back into cells is what the device must write.

CURVE_X: points of y^2 = x^3 + 3 whose STORED x is (top << 224) | (2^224 - 1), limbs 0 ... 6 all ones, so two of them differ in the
top limb only; CURVE_X_PLAIN the same for the plain x a params file holds.  NEAR_MISS: a point off the curve whose stored y^2 and
x^3 + 3 differ in the top limb only -- what an equality test that skipped that limb would take for a point."""
import functools

import test_field_headers as fh

FR, FQ, CARRIES = fh.FR, fh.FQ, fh.CARRIES
N_OPERANDS = 64
LOW_ONES = (1 << 224) - 1
TOPS = (0x30644e71, 1)  # the top limb of a borrow-chain pattern: the largest a canonical value of either field has, and 1


def named(field):
    """the operands chosen by name, in order, each once (1 << 224 is named twice: as a borrow-chain pattern and on its own)"""
    m = field.m
    values = list(field.special) + list(CARRIES) + [(m + 1) // 2, m - field.one]
    for top in TOPS:
        values += [top << 224, (top << 224) | 1]  # a borrow out of limb 0 runs through seven zero limbs
    values += [1 << 32, (1 << 32) - 1, 1 << 224]
    return list(dict.fromkeys(values))


@functools.lru_cache(maxsize=None)
def OPERANDS(field):
    """64 distinct canonical raw values: the named ones, then seeded values of the field"""
    first = named(field)
    rest = [v for v in field.random(N_OPERANDS) if v not in first]
    return tuple(first + rest[:N_OPERANDS - len(first)])


def plain(field, raw):
    """the value the raw pattern is the cell of"""
    return raw * field.r_inv % field.m


def plains(field, raws):
    return [plain(field, w) for w in raws]


@functools.lru_cache(maxsize=None)
def pairs(field):
    """the 4 096 ordered pairs (x, y) of the operands, x the slower index"""
    ops = OPERANDS(field)
    return tuple((x, y) for x in ops for y in ops)


def pair_columns(field=FR):
    """(xs, ys): four columns of 1 024 raw values each, pair 1024 c + i at row i of column c"""
    p = pairs(field)
    cut = lambda which: [[q[which] for q in p[c:c + 1024]] for c in range(0, len(p), 1024)]  # noqa: E731
    return cut(0), cut(1)


def ntt_pair_columns(field=FR):
    """eight columns of 2^10 raw coefficients: pair 512 c + j has x at coefficient j and y at coefficient j + 512 of column c, the two
    that a bit-reversed load puts side by side for the first, twiddle-free butterfly"""
    p = pairs(field)
    return [[q[0] for q in p[c:c + 512]] + [q[1] for q in p[c:c + 512]] for c in range(0, len(p), 512)]


def cycled(field, rows, step=1, first=0):
    """`rows` raw values, the operands in order from `first` by `step`, round and round"""
    ops = OPERANDS(field)
    return [ops[(first + step * i) % N_OPERANDS] for i in range(rows)]


# ---- the curve -----------------------------------------------------------------------------------------------------------------------

def curve_points(stored, count=4, tops=40):
    """((top, (x, y)) ...): the first `count` of the `tops` patterns (top << 224) | (2^224 - 1), top downward from 0x30644e71, that are the
    x of a point -- the stored x (x * 2^256 mod q has the pattern) or the plain one.  q = 3 mod 4, so a square root is a power."""
    q = FQ.m
    assert q % 4 == 3
    found = []
    for top in range(TOPS[0], TOPS[0] - tops, -1):
        w = (top << 224) | LOW_ONES
        x = plain(FQ, w) if stored else w
        a = (x * x * x + 3) % q
        y = pow(a, (q + 1) // 4, q)
        if y * y % q == a:
            found.append((top, (x, y)))
    return tuple(found[:count]), len(found)


(CURVE_X, CURVE_X_FOUND), (CURVE_X_PLAIN, CURVE_X_PLAIN_FOUND) = curve_points(True), curve_points(False)


def near_miss():
    """((x, y'), stored x^3 + 3, stored y'^2): x of CURVE_X, y' a square root of the value whose cell is that of x^3 + 3 with a low bit of
    the top limb flipped"""
    q = FQ.m
    for _top, (x, _y) in CURVE_X:
        rhs = (x * x * x + 3) * FQ.one % q
        for bit in range(1, 16):
            lhs = rhs ^ (bit << 224)
            t = plain(FQ, lhs)
            y = pow(t, (q + 1) // 4, q)
            if lhs < q and y * y % q == t:
                return (x, y), rhs, lhs
    raise AssertionError("no near miss among the patterns")


NEAR_MISS, NEAR_MISS_RHS, NEAR_MISS_LHS = near_miss()
