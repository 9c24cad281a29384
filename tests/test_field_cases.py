"""tests/field_cases.py without a GPU: the operand set has the properties tests/test_gpu_field_operands.py relies on, the host build
of csrc/aesw_mont.h (tests/field_driver.cpp under g++, the reference of tests/test_field_headers.py) agrees with Python integers on
every ordered pair of the set and on its inverses, and the identities that isolate one device operation hold on the models: a fold
under the plain 1 is an addition, and a column with coefficients only at j and j + 512 transforms to omega^(j i) (x + y) at the even
rows i and omega^(j i) (x - y) at the odd ones -- the pairing of the first butterfly."""
import pytest

import field_cases as fc
import msm_model as mm
import ntt_model as nm
import open_model as om
import test_field_headers as fh

FIELDS = (fc.FR, fc.FQ)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("field_cases")


@pytest.fixture(scope="module")
def driver(tmp):
    return fh.build(tmp)


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.name)
def test_the_set_is_64_distinct_canonical_values_and_holds_every_named_one(field):
    m, ops = field.m, fc.OPERANDS(field)
    assert len(ops) == fc.N_OPERANDS == 64 and len(set(ops)) == 64 and all(0 <= v < m for v in ops)
    want = set(field.special) | set(fc.CARRIES) | {(m + 1) // 2, m - field.one, 1 << 32, (1 << 32) - 1, 1 << 224}
    want |= {top << 224 for top in fc.TOPS} | {(top << 224) | 1 for top in fc.TOPS}
    assert want == set(fc.named(field)) and len(want) == 22 and list(ops[:22]) == fc.named(field)
    assert set(ops[22:]) <= set(field.random(64)) and (field.special + fc.CARRIES) == ops[:14]
    # what each is there for: a sum on m, a difference that borrows through seven zero limbs, a lone top limb
    assert (m + 1) // 2 + (m - 1) // 2 == m and (m - field.one) + field.one == m and (m - 1) + 1 == m
    for top in fc.TOPS:
        assert fh.cells([top << 224])[0, :28].max() == 0 and fh.cells([(top << 224) - 1])[0, :28].min() == 0xFF
    assert nm.MONT == fc.FR.one and mm.MONT_Q == fc.FQ.one and nm.R == fc.FR.m and mm.Q == fc.FQ.m
    assert all(fc.plain(field, v) * field.one % m == v for v in ops)  # the models' to_cells gives the raw pattern back
    if field is fc.FR:
        assert nm.from_cells(fh.cells(ops)) == fc.plains(field, ops) and nm.to_cells(fc.plains(field, ops)).tobytes() == fh.cells(ops).tobytes()


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.name)
def test_the_layouts_hold_every_ordered_pair_once(field):
    ops = fc.OPERANDS(field)
    every = {(x, y) for x in ops for y in ops}
    xs, ys = fc.pair_columns(field)
    assert len(xs) == len(ys) == 4 and all(len(c) == 1024 for c in xs + ys)
    laid = [(x, y) for cx, cy in zip(xs, ys) for x, y in zip(cx, cy)]
    assert len(laid) == 4096 and set(laid) == every
    cols = fc.ntt_pair_columns(field)
    assert len(cols) == 8 and all(len(c) == 1024 for c in cols)
    laid = [(c[j], c[j + 512]) for c in cols for j in range(512)]
    assert len(laid) == 4096 and set(laid) == every
    assert sum(1 for x, y in every if x + y == field.m) >= 8 and sum(1 for x, y in every if x == y) == 64
    assert sum(1 for x, y in every if x != y and x >> 224 == y >> 224) >= 44  # equal in the top limb: the borrow comes from below
    assert fc.cycled(field, 130, 9, 3)[:3] == [ops[3], ops[12], ops[21]] and set(fc.cycled(field, 64, 9)) == set(ops)


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.name)
def test_the_host_build_agrees_with_python_on_every_ordered_pair_and_on_the_inverses(driver, tmp, field):
    p = fc.pairs(field)
    fh.check(driver, tmp, field, [x for x, _y in p], [y for _x, y in p])
    fh.check_inverse(driver, tmp, field, list(fc.OPERANDS(field)))


def test_a_fold_under_the_plain_one_is_an_addition_and_one_without_columns_cells_a_product():
    xs, ys = fc.pair_columns()
    r, one = fc.FR.m, fc.plain(fc.FR, fc.FR.one)
    assert one == 1
    for cx, cy in zip(xs, ys):
        got = nm.to_cells(om.fold([fc.plains(fc.FR, cy)], one, fc.plains(fc.FR, cx)))
        assert got.tobytes() == fh.cells([(x + y) % r for x, y in zip(cx, cy)]).tobytes()
    # c = 0: the cell of plain(x) plain(v) is the Montgomery product of the raw patterns
    ops = fc.OPERANDS(fc.FR)
    for v in ops[:16]:
        got = nm.to_cells(om.fold([[0] * 64], fc.plain(fc.FR, v), fc.plains(fc.FR, ops)))
        assert got.tobytes() == fh.cells([x * v * fc.FR.r_inv % r for x in ops]).tobytes()


def test_coefficients_at_j_and_j_plus_512_meet_in_one_sum_and_one_difference():
    r, k, w = nm.R, 10, nm.omega(10)
    ops = fc.plains(fc.FR, fc.OPERANDS(fc.FR))
    for j, (x, y) in ((0, (ops[3], ops[9])), (1, (ops[14], ops[14])), (511, (ops[5], ops[20])), (77, (ops[0], ops[7]))):
        coeff = [0] * 1024
        coeff[j], coeff[j + 512] = x, y
        got = nm.coeff_to_lagrange(coeff, k)
        assert got == [pow(w, j * i, r) * (x + y if i % 2 == 0 else x - y) % r for i in range(1024)]
        if j == 0:
            assert got[0::2] == [(x + y) % r] * 512 and got[1::2] == [(x - y) % r] * 512
    # the bit-reversed load: slots 2 t and 2 t + 1 hold coefficients j and j + 512
    rev = lambda i: int(format(i, "010b")[::-1], 2)  # noqa: E731
    assert all(rev(2 * t + 1) == rev(2 * t) + 512 and rev(2 * t) < 512 for t in range(512))


def test_the_curve_patterns_are_points_and_differ_in_the_top_limb_only():
    assert fc.CURVE_X_FOUND >= 4 and fc.CURVE_X_PLAIN_FOUND >= 4 and len(fc.CURVE_X) == len(fc.CURVE_X_PLAIN) == 4
    assert [top for top, _p in fc.CURVE_X[:2]] == [0x30644e6f, 0x30644e6d]
    for found, stored in ((fc.CURVE_X, True), (fc.CURVE_X_PLAIN, False)):
        for top, p in found:
            assert mm.on_curve(p) and mm.on_curve(mm.neg(p)) and p[1] != 0
            x = p[0] * mm.MONT_Q % mm.Q if stored else p[0]
            assert x == (top << 224) | fc.LOW_ONES and x < mm.Q
        assert len({top for top, _p in found}) == 4
    a, b = (mm.to_points([p])[0] for _top, p in fc.CURVE_X[:2])
    assert (a[:28] == 0xFF).all() and (a[:28] == b[:28]).all() and (a[28:32] != b[28:32]).any()  # the stored x: equal below the top limb
    # the near miss: off the curve, and the two sides of the curve equation as the device compares them are equal below the top limb
    (x, y), rhs, lhs = fc.NEAR_MISS, fc.NEAR_MISS_RHS, fc.NEAR_MISS_LHS
    assert not mm.on_curve((x, y)) and x == fc.CURVE_X[0][1][0] and 0 <= y < mm.Q
    assert lhs == y * y * mm.MONT_Q % mm.Q and rhs == (x ** 3 + 3) * mm.MONT_Q % mm.Q
    assert lhs != rhs and lhs & ((1 << 224) - 1) == rhs & ((1 << 224) - 1)
