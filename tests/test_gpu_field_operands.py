"""csrc/aesw_mont.h as hipcc compiles it for the device, at the operands where carries and borrows run: the 64 raw limb patterns of
tests/field_cases.py -- 0, 1, m - 1, the Montgomery form of 1, limbs 0 ... 6 all ones, a lone top limb, sums that land on m -- through
the shipped kernels that take cells as they lie, every ordered pair of them, byte for byte against Python integers and the models.

  products       open_fold_kernel (fold_columns without columns' cells: acc * v) and shplonk_combine_kernel (combine_columns)
  sums           open_fold_kernel under the raw Montgomery 1: acc + column
  differences    the first, twiddle-free butterfly of ntt_pass_kernel: coefficients j and j + 512 of a k = 10 column
  powers         open_powers_kernel's 28 squarings and the Horner and join kernels: evaluate_columns, divide_columns at special points
  inverse        grand_invert_kernel: fr_inv, fr_is_zero and the batch of 8, a table of the operands
  Fq             msm_basis_kernel and the bucket, reduce and combine kernels: points whose stored x differ in the top limb only, and a point
                 off the curve whose y^2 and x^3 + 3 differ in the top limb only (fq_eq: the complete addition law compares nothing)

No tolerance anywhere; every output sits in poisoned guard bands (tests/guarded.py); no expectation comes from device code."""
import functools

import numpy as np
import pytest

import field_cases as fc
import grand_model as gm
import guarded as G
import msm_model as mm
import ntt_model as nm
import open_model as om
import shplonk_model as sm
import test_field_headers as fh

pytestmark = pytest.mark.gpu
FR, K, N = fc.FR, 10, 1 << 10
R = FR.m
OPS = fc.OPERANDS(FR)


def put(arena, name, array):
    """a guarded, 16-byte aligned device copy of a uint8 array"""
    import torch
    t = arena.out(name, array.size, array.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(array)).to(t.device))
    return t


def raw_cells(values):
    """uint8 [len, 32]: raw patterns as they lie in memory"""
    return fh.cells(values).copy()


def cells_of_plain(values):
    return nm.to_cells(values)


def new_column(arena, name):
    return arena.out(name, 32 * N, (N, 32))


# ---- products ------------------------------------------------------------------------------------------------------------------------

def test_every_product_of_two_operands_through_the_fold(ctx):
    xs = fc.cycled(FR, N)  # the 64 operands, 16 times over
    arena = G.DeviceArena()
    d_acc, d_zero, d_v = put(arena, "acc", raw_cells(xs)), put(arena, "zero", np.zeros((1, N, 32), np.uint8)), put(arena, "v", raw_cells(OPS))
    got = [ctx.fold_columns(d_zero, K, d_v[i], acc=d_acc, out=new_column(arena, "out%d" % i)) for i in range(len(OPS))]
    arena.check()
    for v, out in zip(OPS, got):
        G.assert_bytes("mont_mul(x, %#x) over the operands x" % v, out.cpu().numpy(), raw_cells([x * v * FR.r_inv % R for x in xs]))
    G.assert_bytes("the accumulator is left alone", d_acc.cpu().numpy(), raw_cells(xs))
    assert {R - 1, FR.one, 0} <= set(OPS)  # (m - 1)^2 and the products with the Montgomery 1 and with 0 are among the pairs


LOW = (R - 1, FR.one, fc.CARRIES[0], 1 << 253, R - FR.one, (R + 1) // 2, 0, 1)


@pytest.mark.parametrize("n_cols,with_acc", ((1, False), (2, False), (1, True), (2, True)), ids=("one", "two", "one-acc", "two-acc"))
def test_every_product_of_two_operands_through_the_combine(ctx, n_cols, with_acc):
    cols = [fc.cycled(FR, N), [OPS[(i + i // 64 + 1) % 64] for i in range(N)]][:n_cols]
    acc = fc.cycled(FR, N, 9, 3) if with_acc else None
    arena = G.DeviceArena(G.CANARIES[with_acc])
    d_cols = put(arena, "cols", np.stack([raw_cells(c) for c in cols]))
    d_acc = put(arena, "acc", raw_cells(acc)) if with_acc else None
    coefs = [[OPS[i], OPS[(5 * i + 2) % 64]][:n_cols] for i in range(len(OPS))]
    got = [ctx.combine_columns(d_cols, K, raw_cells(c), low=raw_cells(LOW), acc=d_acc, out=new_column(arena, "out%d" % i)) for i, c in enumerate(coefs)]
    arena.check()
    plain_cols, plain_low = [fc.plains(FR, c) for c in cols], fc.plains(FR, LOW)
    plain_acc = fc.plains(FR, acc) if with_acc else None
    for c, out in zip(coefs, got):
        exp = cells_of_plain(sm.combine(plain_cols, fc.plains(FR, c), plain_low, plain_acc))
        raw = [((a if with_acc else 0) + sum(v * col[i] * FR.r_inv for v, col in zip(c, cols)) + (LOW[i] if i < 8 else 0)) % R
               for i, a in enumerate(acc or [0] * N)]
        assert exp.tobytes() == raw_cells(raw).tobytes()  # the model on plain values and the integers on raw limbs say the same
        G.assert_bytes("combine under %r" % ([hex(v) for v in c],), out.cpu().numpy(), exp)


# ---- sums ----------------------------------------------------------------------------------------------------------------------------

def test_every_sum_of_two_operands_through_a_fold_under_one(ctx):
    xs, ys = fc.pair_columns()
    arena = G.DeviceArena(G.CANARIES[1])
    d_one = put(arena, "one", raw_cells([FR.one]))
    on_m = 0
    for c, (cx, cy) in enumerate(zip(xs, ys)):
        d_acc, d_col = put(arena, "x%d" % c, raw_cells(cx)), put(arena, "y%d" % c, raw_cells(cy).reshape(1, N, 32))
        got = ctx.fold_columns(d_col, K, d_one.view(32), acc=d_acc, out=new_column(arena, "sum%d" % c))
        arena.check()
        got = got.cpu().numpy()
        G.assert_bytes("mont_add over pairs %d ..." % (1024 * c), got, raw_cells([(x + y) % R for x, y in zip(cx, cy)]))
        for i, (x, y) in enumerate(zip(cx, cy)):
            if x + y == R:  # the sum lands on m exactly: the 32 zero bytes of a zero cell
                on_m += 1
                assert not got[i].any(), (hex(x), hex(y))
    assert on_m >= 8


# ---- differences ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ntt_world():
    """(raw columns [8, 1024, 32], name -> expected cells) by the model, once"""
    cols = fc.ntt_pair_columns()
    plain = [fc.plains(FR, c) for c in cols]
    exp = {name: np.stack([cells_of_plain(getattr(nm, name)(c, K)) for c in plain]) for name in ("coeff_to_lagrange", "lagrange_to_coeff")}
    return np.stack([raw_cells(c) for c in cols]), plain, exp


@pytest.mark.parametrize("in_place", (False, True), ids=("out", "in-place"))
@pytest.mark.parametrize("name", ("coeff_to_lagrange", "lagrange_to_coeff"))
def test_every_difference_and_sum_meets_in_the_first_butterfly(ctx, name, in_place):
    cells, _plain, exp = ntt_world()
    tables = ctx.ntt_tables(K)
    arena = G.DeviceArena(G.CANARIES[in_place])
    d_in = put(arena, "in", cells)
    got = getattr(ctx, name)(d_in, K, tables, out=d_in if in_place else arena.out("out", cells.size, cells.shape))
    arena.check()
    G.assert_bytes("%s over the pair columns, in_place=%s" % (name, in_place), got.cpu().numpy(), exp[name])
    if not in_place:
        G.assert_bytes("the input is left alone", d_in.cpu().numpy(), cells)


@pytest.mark.parametrize("sel", (0, 1))
def test_the_pair_columns_extend_to_the_coset(ctx, sel):
    cells, plain, _exp = ntt_world()
    ext_k = 12
    tables = ctx.ntt_tables(ext_k)
    arena = G.DeviceArena(G.CANARIES[sel])
    got = ctx.coeff_to_extended(put(arena, "coeff", cells[:2]), K, ext_k, tables, zeta_sel=sel, out=arena.out("ext", 2 * (32 << ext_k), (2, 1 << ext_k, 32)))
    arena.check()
    G.assert_bytes("coeff_to_extended, zeta_sel=%d" % sel, got.cpu().numpy(), np.stack([cells_of_plain(nm.coeff_to_extended(c, K, ext_k, sel)) for c in plain[:2]]))


# ---- powers, evaluation, division ----------------------------------------------------------------------------------------------------

POINTS = (0, 1, FR.one, R - 1) + fc.CARRIES + (1 << 253,)  # raw: the zero cell, the cell whose limbs are 1, 0 ... 0, the Montgomery 1, and the rest
N_POINTS = len(POINTS)
POWER_COLS = 10  # X^(2^s), s = 0 ... 9: what open_powers_kernel's squarings of z leave behind, read through an evaluation


def open_workspace(pkg, arena, n_cols, n_points):
    return arena.out("ws", int(pkg.api.load_open_library().aesw_open_workspace_bytes(K, n_cols, n_points)))


def test_evaluation_at_special_points_of_a_special_column_and_of_the_powers_of_x(pkg, ctx):
    column = fc.plains(FR, fc.cycled(FR, N, 9, 5))
    powers = [[1 if i == 1 << s else 0 for i in range(N)] for s in range(POWER_COLS)]
    cols = [column] + powers
    cells = np.stack([cells_of_plain(c) for c in cols])
    assert cells[0].tobytes() == raw_cells(fc.cycled(FR, N, 9, 5)).tobytes() and N_POINTS == 10 and all(p < R for p in POINTS)
    zs = fc.plains(FR, POINTS)
    arena = G.DeviceArena()
    d_coeff = put(arena, "coeff", cells)
    got = ctx.evaluate_columns(d_coeff, K, put(arena, "points", raw_cells(POINTS)), out=arena.out("evals", len(cols) * N_POINTS * 32, (len(cols), N_POINTS, 32)),
                               _workspace=open_workspace(pkg, arena, len(cols), N_POINTS))
    arena.check()
    got = got.cpu().numpy()
    G.assert_bytes("the special column at the special points", got[0], cells_of_plain([om.evaluate(column, z) for z in zs]))
    for s in range(POWER_COLS):
        G.assert_bytes("z^(2^%d)" % s, got[1 + s], cells_of_plain([pow(z, 1 << s, R) for z in zs]))
    G.assert_bytes("the model says the same of the powers", got[1:], cells_of_plain([om.evaluate(c, z) for c in powers for z in zs]).reshape(POWER_COLS, N_POINTS, 32))
    G.assert_bytes("the columns are left alone", d_coeff.cpu().numpy(), cells)


@pytest.mark.parametrize("in_place", (False, True), ids=("out", "in-place"))
def test_division_at_special_points_of_a_special_column(pkg, ctx, in_place):
    raw = [fc.cycled(FR, N, 9, 5), fc.cycled(FR, N, 1, 0)]
    cols = [fc.plains(FR, c) for c in raw]
    cells = np.stack([raw_cells(c) for c in raw])
    for i, z_raw in enumerate(POINTS):
        z = fc.plain(FR, z_raw)
        pairs = [om.divide(c, z) for c in cols]
        arena = G.DeviceArena(G.CANARIES[i % 2])
        d_coeff = put(arena, "coeff", cells)
        quot, rem = ctx.divide_columns(d_coeff, K, raw_cells([z_raw]), out=d_coeff if in_place else arena.out("quot", cells.size, cells.shape),
                                       _rem=arena.out("rem", 64, (2, 32)), _workspace=open_workspace(pkg, arena, 2, 1))
        arena.check()
        G.assert_bytes("the quotient at raw %#x" % z_raw, quot.cpu().numpy(), np.stack([cells_of_plain(q) for q, _rem in pairs]))
        G.assert_bytes("the remainder at raw %#x" % z_raw, rem.cpu().numpy(), cells_of_plain([rem for _q, rem in pairs]))


# ---- the inverse ---------------------------------------------------------------------------------------------------------------------

BATCH = 8  # grand_invert_kernel: a lane inverts rows 8 b ... 8 b + 7 of one table with one fr_inv; 66 561 = 8 * 8 320 + 1
TABLE_SHIFT = (0, 3, 7)  # per table: row 66 560, alone in the last batch, holds 0, m - 1 and the Montgomery 1
ZERO_BATCH = (100, 4000, 8319)  # per table: a batch whose eight cells are the zero cell: fr_inv of the Montgomery 1
X_INDEX = 9  # CARRIES[0]: the operand that beta = m - x brings to zero
X_BATCH = (101, 4001, 8318)  # per table: a batch of eight x


@functools.lru_cache(maxsize=None)
def invert_index():
    """int [3, 66561]: which operand lies at every row.  Row i = 8 b + p holds operand 9 b + p + shift mod 64, so over 64 consecutive
    batches every position p meets every operand, zero among them"""
    i = np.arange(gm.BINS)
    idx = np.stack([(9 * (i // BATCH) + i % BATCH + shift) % 64 for shift in TABLE_SHIFT])
    for t in range(3):
        idx[t, BATCH * ZERO_BATCH[t]:BATCH * ZERO_BATCH[t] + BATCH] = 0
        idx[t, BATCH * X_BATCH[t]:BATCH * X_BATCH[t] + BATCH] = X_INDEX
    return idx


def raw_cell(value):
    import torch
    return torch.from_numpy(raw_cells([value])[0]).cuda()


def test_the_inverse_table_is_laid_out_as_the_batches_need_it():
    idx = invert_index()
    assert OPS[0] == 0 and OPS[X_INDEX] == fc.CARRIES[0] and gm.BINS == 8 * 8320 + 1 and gm.R == R
    for t in range(3):
        whole = idx[t, :8 * 8320].reshape(8320, 8)
        for p in range(8):
            assert set(whole[:, p].tolist()) == set(range(64))  # every position of a batch meets zero and every special
        assert not whole[ZERO_BATCH[t]].any() and (whole[X_BATCH[t]] == X_INDEX).all()
    assert [OPS[int(j)] for j in idx[:, gm.BINS - 1]] == [0, R - 1, FR.one]  # the last, partial batch holds a special


@pytest.mark.parametrize("case", ("beta-zero", "sums-on-m", "gamma-carries"))
def test_the_inverse_of_every_operand_in_every_position_of_a_batch(pkg, ctx, case):
    import torch
    # raw challenges: beta = 0 leaves the table's own cells; beta = m - x and gamma = m - 1 bring x and 1 to a sum of exactly m
    beta, gamma = {"beta-zero": (0, OPS[20]), "sums-on-m": (R - OPS[X_INDEX], R - 1), "gamma-carries": (OPS[30], fc.CARRIES[1])}[case]
    idx = invert_index()
    table = raw_cells(OPS)[idx]
    exp, zeros = [], 0
    for c in (beta, gamma):  # one inverse per distinct sum: gm.inv's memo, at most 64 a plane
        sums = [(w + c) % R for w in OPS]
        lut = gm.cells([gm.inv(fc.plain(FR, s)) for s in sums])
        exp.append(lut[idx])
        zeros += int(np.isin(idx, [j for j, s in enumerate(sums) if s == 0]).sum())
    exp = np.stack(exp)
    arena = G.DeviceArena(G.CANARIES[len(case) % 2])
    d_table = put(arena, "table", table)
    out, rep = arena.out("inv", 2 * 3 * gm.BINS * 32, (2, 3, gm.BINS, 32)), arena.out("report", 24)
    d_beta, d_gamma = raw_cell(beta), raw_cell(gamma)  # named: a temporary's memory is handed out again before the kernel reads it
    rc = pkg.api.load_grand_library().aesw_grand_invert_table_device(ctx._h, d_table.data_ptr(), d_beta.data_ptr(), d_gamma.data_ptr(), out.data_ptr(), rep.data_ptr(),
                                                                     ctx._stream())
    assert rc == 0, (rc, ctx._lib.aesw_last_error(ctx._h))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.argwhere((got != exp).any(axis=3))
    assert not bad.size, "%s: %d cells differ, first (plane, table, row) %r: the inverse of raw %#x" % (
        case, len(bad), bad[0].tolist(), (OPS[int(idx[bad[0][1], bad[0][2]])] + (beta, gamma)[bad[0][0]]) % R)
    assert pkg.api.grand_invert_report_dict(rep.view(torch.int64)) == {"cells": 2 * 3 * gm.BINS, "noncanonical": False, "zero_terms": zeros}
    if case == "beta-zero":
        assert zeros == int((idx == 0).sum()) >= 3 * 8 + 3 * 1000 and not got[0][idx == 0].any()
        one_at = idx == OPS.index(FR.one)
        assert (got[0][one_at] == raw_cells([FR.one])[0]).all()  # the Montgomery 1 is its own inverse
    if case == "sums-on-m":
        assert zeros == int((idx == X_INDEX).sum()) + int((idx == 1).sum()) and not got[0][idx == X_INDEX].any() and not got[1][idx == 1].any()
        assert got[0][idx != X_INDEX].any(axis=1).all()
    if case == "gamma-carries":
        assert zeros == 0 and got.reshape(-1, 32).any(axis=1).all()
    G.assert_bytes("the table is left alone", d_table.cpu().numpy(), table)
    arena.check_on_device()


# ---- Fq ------------------------------------------------------------------------------------------------------------------------------

P = tuple(p for _top, p in fc.CURVE_X)  # four points whose stored x is ones below the top limb
SPECIAL_ROWS = P + tuple(mm.neg(p) for p in P) + (P[0],)  # rows 0 ... 3, their negatives at 4 ... 7, P_0 again at 8


@functools.lru_cache(maxsize=None)
def special_basis():
    return SPECIAL_ROWS + mm.known_basis(N)[len(SPECIAL_ROWS):]


def test_the_basis_call_converts_points_of_special_coordinates_and_refuses_a_near_miss(pkg, ctx):
    plain = tuple(p for _top, p in fc.CURVE_X_PLAIN)
    points = plain + tuple(mm.neg(p) for p in plain) + SPECIAL_ROWS
    points = points + mm.known_basis(N)[len(points):]
    canonical = mm.canonical_points(points)
    assert (canonical[0, :28] == 0xFF).all() and (canonical[:4, :28] == canonical[0, :28]).all() and len(points) == N
    arena = G.DeviceArena()
    report = arena.out("report", 16)
    got = ctx.msm_basis(put(arena, "points", canonical), out=arena.out("basis", canonical.size, canonical.shape), _report=report)  # raises on a bad point
    arena.check()
    G.assert_bytes("the basis", got.cpu().numpy(), mm.to_points(points))
    assert [int(v) for v in report.cpu().numpy().view(np.uint64)][0] == 0
    stored = got.cpu().numpy()[8:12, :32]
    assert (stored[:, :28] == 0xFF).all()  # the CURVE_X rows came out as the patterns they were chosen for
    # off the curve by the top limb alone: y^2 and x^3 + 3 are equal in limbs 0 ... 6, and the point is refused at its index
    for at in (0, 517, N - 1):
        bad = canonical.copy()
        bad[at] = mm.canonical_points([fc.NEAR_MISS])[0]
        with pytest.raises(pkg.AeswError, match="1 of the 2\\^10 points .* index %d$" % at):
            ctx.msm_basis(bad)


def commit(pkg, ctx, arena, kind, scalars, basis, slices):
    n_cols = scalars.shape[0]
    ws = arena.out("ws", int(pkg.api.load_msm_library().aesw_msm_workspace_bytes(K, n_cols, kind, slices)))
    got = ctx.commit_columns(put(arena, "scalars", scalars), basis, out=arena.out("out", n_cols * 64, (n_cols, 64)), slices=slices, _workspace=ws)
    arena.check()
    return got.cpu().numpy()


def sparse(rows, kind_cells):
    """a column of N scalars, zero but for rows: {row: value}"""
    col = np.zeros((N, 32) if kind_cells else (N,), np.uint8)
    for row, value in rows.items():
        col[row] = raw_cells([value])[0] if kind_cells else value
    return col


@pytest.mark.parametrize("slices", (0, 1, 3))
def test_commitments_over_points_whose_x_differ_in_the_top_limb_only(pkg, ctx, slices):
    import torch
    basis = special_basis()
    d_basis = torch.from_numpy(mm.to_points(basis)).cuda()
    selections = [(i,) for i in range(8)] + [(0, 8), (0, 4), (0, 1), (1, 2, 3), tuple(range(9)), (0, 1, 600), (4, 5, 1023)]
    got = commit(pkg, ctx, G.DeviceArena(G.CANARIES[slices % 2]), 1, np.stack([sparse({r: 1 for r in rows}, False) for rows in selections]), d_basis, slices)
    for rows, cell in zip(selections, got):
        G.assert_bytes("rows %r, slices=%d" % (rows, slices), cell, mm.to_points([mm.msm([1] * len(rows), [basis[r] for r in rows])])[0])
    assert mm.from_points(got[8]) == [mm.add(P[0], P[0])] and not got[9].any()  # P + P doubles; P + (-P) is 64 zero bytes
    assert mm.from_points(got[12]) == [P[0]]
    # Fr cells: a few rows whose stored cell is special, over the special points and two of the known basis
    columns = [{0: fc.CARRIES[0], 1: R - 1, 5: 1 << 253, 700: fc.CARRIES[0]}, {0: R - 1, 8: 1, 4: 1 << 253}, {1: FR.one, 2: FR.one, 1023: fc.CARRIES[0]},
               {0: FR.one, 4: FR.one}]
    got = commit(pkg, ctx, G.DeviceArena(G.CANARIES[1 - slices % 2]), 0, np.stack([sparse(rows, True) for rows in columns]), d_basis, slices)
    for rows, cell in zip(columns, got):
        exp = mm.msm([fc.plain(FR, w) for w in rows.values()], [basis[r] for r in rows])
        G.assert_bytes("cells %r, slices=%d" % ({r: hex(w) for r, w in rows.items()}, slices), cell, mm.to_points([exp])[0])
    assert not got[3].any()
