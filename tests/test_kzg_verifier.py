"""The proof stage under a verifier, without a GPU.

tests/kzg_verifier.py plays the party no other test plays: it knows the commitments, the claimed evaluations, the challenges and
the prover's two points, and none of the prover's tables.  Against a basis tau^i G of known tau a commitment is f(tau) G, so every
commitment here is made by its exponent -- one Horner sum and one fixed-base multiplication -- and the wide set of
sc.full_stage() costs evaluations, not multi-scalar products.

  completeness   the verifier accepts tests/shplonk_model.py's opening of sc.stage(10), of sc.full_stage() (16 sets, t = 1 ... 8,
                 257 columns in one set), of the stages with y, v at 0 and 1 and of u inside set 0; where z_0 = 0 (the device
                 reports z0_zero) it refuses by that name and divides by nothing
  soundness      one evaluation raised by 1 in each set, H + G, W + G, two commitments of a set swapped, two sets' evaluations
                 swapped, u + 1: each is rejected by the equation, not by a shape
  the driver     tests/shplonk_driver.cpp -- csrc/aesw_shplonk.h's own lines on the CPU -- gives an h and a W the verifier accepts
  the bytes      a whole stage through transcript_model: read_proof recomputes x, y, v, u from the proof alone
  the bases      tau_basis and lagrange_basis against msm_model's double-and-add, and against each other
  independence   kzg_verifier imports neither shplonk_model nor open_model"""
import ast
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kzg_verifier as kv
import msm_model as mm
import ntt_model as nm
import shplonk_cases as sc
import shplonk_model as sm
import transcript_model as tm
from test_gpu_shplonk_chain import QUERIES

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
R, G1, TAU = nm.R, mm.GENERATOR, kv.TAU
K = 10
WRONG = ((0, 3, 0), (1, 0, 1), (2, 0, 1), (3, 4, 7))  # one evaluation in each set of sc.SETS
TWIN_SETS = (((0, 1), 1), ((2, 3), 1), ((4,), 2))     # two sets of one shape, so that their evaluations can change places


def stages():
    return {"stage": sc.stage(K), "full": sc.full_stage(), "twins": sc.stage(K, sets=TWIN_SETS), **sc.u_on_a_point(), **sc.degenerate_stages(K),
            **{"wrong%d" % i: sc.stage(K, wrong=w) for i, w in enumerate(WRONG)}}


@functools.lru_cache(maxsize=None)
def opened(name):
    p, pts, columns, evals, y, v, u = stages()[name]
    return sm.opening(p, columns, evals, pts, y, v, lambda _h: u)


@functools.lru_cache(maxsize=None)
def committed(name):
    """(the commitments of the stage's columns, [h], [W]), each by its exponent"""
    columns = stages()[name][2]
    own = "full" if columns is sc.full_stage()[2] else "stage" if columns is sc.stage(K)[2] else name  # the columns are shared: commit them once
    of_columns = committed(own)[0] if own != name else [[kv.commit(c) for c in of_set] for of_set in columns]
    o = opened(name)
    return of_columns, kv.commit(o["h"]), kv.commit(o["w"])


OWN = object()  # None is a point, the identity


def verdict(name, commitments=None, evals=None, u=None, H=OWN, W=OWN):
    """the verifier on the named stage, with whatever is given in place of the prover's own"""
    p, pts, _columns, own_evals, y, v, own_u = stages()[name]
    C, h, w = committed(name)
    return kv.verify_shplonk(p, C if commitments is None else commitments, own_evals if evals is None else evals, pts, y, v, own_u if u is None else u,
                             h if H is OWN else H, w if W is OWN else W, TAU)


# ---- completeness -----------------------------------------------------------------------------------------------------------------------

def test_the_verifier_accepts_the_models_opening_of_the_stage():
    assert opened("stage")["report"] == dict(bad_sets=0, first_bad_set=None, zero_differences=0, z0_zero=0, last_remainder=0)
    got = verdict("stage")
    assert got and got.accepted and got.reason is None, got
    C, h, w = committed("stage")
    assert None not in [c for of_set in C for c in of_set] + [h, w] and h != w and all(mm.on_curve(c) for of_set in C for c in of_set)


def test_the_verifier_accepts_the_full_plan_and_u_inside_set_0():
    p = sc.full_stage()[0]
    assert len(p.sets) == 16 and sorted(set(p.set_points)) == list(range(1, 9)) and max(p.set_cols) == sc.WIDE_COLS == 257
    got = verdict("full")
    assert got, got
    assert opened("u_inside_set_0")["fin"]["z_t"] == 0 and opened("u_inside_set_0")["report"]["z0_zero"] == 0
    assert verdict("u_inside_set_0"), "z_T = 0 alone: h drops out of L, and the opening stands"
    # and it is not a verifier that accepts anything at this size: one evaluation of the wide set, and of the last set, raised by 1
    for i, j, s in ((sc.WIDE_SET, 256, 0), (15, 0, 7)):
        evals = [[list(e) for e in of_set] for of_set in sc.full_stage()[3]]
        evals[i][j][s] = (evals[i][j][s] + 1) % R
        assert verdict("full", evals=evals).reason == "equation", (i, j, s)


@pytest.mark.parametrize("name", sorted(sc.degenerate_stages(K)))
def test_challenges_of_0_and_1_are_accepted_and_z0_zero_is_refused_by_name(name):
    o = opened(name)
    got = verdict(name)
    if name.endswith(",u=0"):  # u is super-set point 0, outside set 0: the device reports z0_zero, the verifier refuses and divides by nothing
        assert o["report"]["z0_zero"] == 1 and not got and got.reason == "z0_zero", got
    else:
        assert o["report"]["z0_zero"] == 0 and got, got


def test_u_on_a_point_outside_set_0_is_refused_by_name():
    assert opened("u_outside_set_0")["report"]["z0_zero"] == 1
    got = verdict("u_outside_set_0")
    assert not got and got.reason == "z0_zero" and "z0_zero" in repr(got), got
    # whatever the two points are: the refusal comes before any group operation
    assert verdict("u_outside_set_0", H=None, W=G1).reason == "z0_zero"


def test_two_equal_points_in_a_set_are_refused_by_name():
    p, pts, _columns, evals, y, v, u = sc.stage(K)
    pts = list(pts)
    pts[6] = pts[5]  # set 3 holds both: no interpolant, and no inverse of their difference
    C, h, w = committed("stage")
    got = kv.verify_shplonk(p, C, evals, pts, y, v, u, h, w, TAU)
    assert not got and got.reason == "repeated_point"


# ---- soundness --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(WRONG)))
def test_one_evaluation_raised_by_1_is_rejected(case):
    i, j, s = WRONG[case]
    name = "wrong%d" % case
    assert [x[0] for x in WRONG] == list(range(len(sc.SETS))) and stages()[name][3][i][j][s] == (sc.stage(K)[3][i][j][s] + 1) % R
    # the prover that opens from the wrong value: its report names the set, and the verifier rejects what it made
    assert opened(name)["report"]["first_bad_set"] == i and opened(name)["report"]["last_remainder"] != 0
    assert verdict(name).reason == "equation"
    assert verdict("stage", evals=stages()[name][3]).reason == "equation"  # the honest prover's points under the wrong value
    # R_i lies below Z_i's degree and the last division drops its remainder, so the wrong value moves neither h nor W: the points
    # this prover made are the honest ones, and under the right evaluations they stand
    assert committed(name)[1:] == committed("stage")[1:] and verdict(name, evals=sc.stage(K)[3])


def test_h_and_w_moved_by_the_generator_are_rejected():
    _C, h, w = committed("stage")
    assert verdict("stage", H=mm.add(h, G1)).reason == "equation" and verdict("stage", W=mm.add(w, G1)).reason == "equation"
    assert verdict("stage", H=w, W=h).reason == "equation" and verdict("stage", H=None).reason == "equation" and verdict("stage", W=None).reason == "equation"


def test_two_commitments_of_a_set_swapped_are_rejected():
    C, _h, _w = committed("stage")
    swapped = [list(of_set) for of_set in C]
    swapped[0][0], swapped[0][1] = swapped[0][1], swapped[0][0]
    assert C[0][0] != C[0][1] and verdict("stage", commitments=swapped).reason == "equation"
    swapped = [list(of_set) for of_set in C]
    swapped[3][3], swapped[3][4] = swapped[3][4], swapped[3][3]
    assert verdict("stage", commitments=swapped).reason == "equation"


def test_two_sets_evaluations_swapped_are_rejected():
    assert verdict("twins"), "the plan of two sets of one shape, as the prover made it"
    evals = [[list(e) for e in of_set] for of_set in stages()["twins"][3]]
    evals[0], evals[1] = evals[1], evals[0]
    assert verdict("twins", evals=evals).reason == "equation"  # the shapes agree: it is the equation that fails
    C, _h, _w = committed("twins")
    assert verdict("twins", commitments=[C[1], C[0], C[2]]).reason == "equation"


def test_another_u_is_rejected():
    u = sc.stage(K)[6]
    assert verdict("stage", u=(u + 1) % R).reason == "equation" and verdict("stage", u=(u - 1) % R).reason == "equation"
    p, pts, _columns, evals, y, v, _u = sc.stage(K)
    C, h, w = committed("stage")
    assert kv.verify_shplonk(p, C, evals, pts, (y + 1) % R, v, u, h, w, TAU).reason == "equation" and kv.verify_shplonk(p, C, evals, pts, y, (v + 1) % R, u, h, w, TAU).reason == "equation"
    assert kv.verify_shplonk(p, C, evals, pts, y, v, u, h, w, TAU + 1).reason == "equation"  # and another tau is another basis


def test_a_malformed_statement_is_refused_as_a_shape():
    C, _h, _w = committed("stage")
    evals = sc.stage(K)[3]
    assert verdict("stage", commitments=C[:3]).reason == "shape" and verdict("stage", evals=evals[:3]).reason == "shape"
    assert verdict("stage", commitments=[C[0][:4]] + C[1:]).reason == "shape" and verdict("stage", evals=[evals[1]] + evals[1:]).reason == "shape"


# ---- one opening ------------------------------------------------------------------------------------------------------------------------

def test_verify_single_accepts_a_quotient_and_rejects_a_moved_evaluation():
    coeff = nm.seeded_values(64, 0x73696e67)
    for x in (nm.seeded_values(1, 0x78)[0], 0, nm.omega(6)):
        quot, s = [0] * len(coeff), 0  # synthetic division from the top
        for i in range(len(coeff) - 1, -1, -1):
            quot[i], s = s, (coeff[i] + x * s) % R
        assert s == kv.evaluate(coeff, x)
        C, Wq = kv.commit(coeff), kv.commit(quot)
        assert kv.verify_single(C, x, s, Wq) and not kv.verify_single(C, x, (s + 1) % R, Wq) and not kv.verify_single(C, (x + 1) % R, s, Wq)
        assert not kv.verify_single(mm.add(C, G1), x, s, Wq) and not kv.verify_single(C, x, s, mm.add(Wq, G1))


# ---- the CPU driver: the header's own lines under the verifier --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("kzg_driver")
    exe = d / "shplonk_driver"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-I", str(CSRC), str(ROOT / "tests" / "shplonk_driver.cpp"), "-o", str(exe)], check=True)

    def run(stage, k):
        """(h, W, the report's first four words) of the driver's run of the stage"""
        p, pts, columns, evals, y, v, u = stage
        (d / "plan.txt").write_text(p.text())
        nm.to_cells(pts + [y, v, u] + sc.flat_evals(evals) + [c for of_set in columns for column in of_set for c in column]).tofile(d / "cells.bin")
        for args in (["constants"], ["stage", k, d / "plan.txt", d / "cells.bin", d / "out.bin"]):
            out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
            assert out.returncode == 0, (args, out.stderr[-2000:])
            if args == ["constants"]:
                y_pow_at = int(out.stdout.split()[12])
        raw, n = np.fromfile(d / "out.bin", np.uint8), 1 << k
        at = y_pow_at + max(p.set_cols) + len(p.sets) * (n + 8)  # the scalars block, then N_i and its eight remainder cells per set
        assert raw.size == 32 * (at + 3 * n) + 64
        take = lambda first: nm.from_cells(raw[32 * first:32 * (first + n)].reshape(n, 32))  # noqa: E731
        return take(at), take(at + 2 * n), [int(w) for w in raw[32 * (at + 3 * n):].view("<u8")[:4]]
    return run


def test_the_drivers_h_and_w_are_accepted_and_those_of_a_wrong_evaluation_are_not(driver):
    h, w, report = driver(sc.stage(K), K)
    assert report == [0, (1 << 64) - 1, 0, 0] and any(h) and any(w)
    assert verdict("stage", H=kv.commit(h), W=kv.commit(w)), "the header's own lines, run on the CPU, do not satisfy the verifier"
    h, w, report = driver(stages()["wrong2"], K)
    assert report[:2] == [1, 2]
    assert verdict("wrong2", H=kv.commit(h), W=kv.commit(w)).reason == "equation"


def test_the_drivers_full_plan_is_accepted(driver):
    h, w, report = driver(sc.full_stage(), sc.FULL_K)
    assert report == [0, (1 << 64) - 1, 0, 0]
    assert verdict("full", H=kv.commit(h), W=kv.commit(w))


# ---- the bytes --------------------------------------------------------------------------------------------------------------------------

def chain_plan():
    """api.multiopen_plan(QUERIES), as tests/test_gpu_shplonk_chain.py pins it"""
    plan = sc.Plan((0, 1, -1), [((0,), ["advice"]), ((0, 1), ["z"]), ((0, 1, 2), ["z2", "advice2"])])
    assert sorted((c, plan.rotations[q]) for idx, cols in plan.sets for c in cols for q in idx) == sorted(QUERIES)
    return plan


def proved(bump=None):
    """the proof bytes of a whole stage by the models: commitments, x, evaluations, then shplonk_model.opening between y, v and u"""
    plan = chain_plan()
    columns = [[nm.seeded_values(1 << K, 0x6b7a + 16 * i + j) for j in range(len(cols))] for i, (_idx, cols) in enumerate(plan.sets)]
    t = tm.Transcript().write_points([kv.commit(c) for of_set in columns for c in of_set])
    points = kv.rotated(t.squeeze(), K, plan.rotations)
    evals = [[[kv.evaluate(c, points[q]) for q in idx] for c in columns[i]] for i, (idx, _cols) in enumerate(plan.sets)]
    if bump is not None:
        i, j, s = bump
        evals[i][j][s] = (evals[i][j][s] + 1) % R
    t.write_scalars(sc.flat_evals(evals))
    y, v = t.squeeze(), t.squeeze()

    def u_of(h):
        t.write_points([kv.commit(h)])
        return t.squeeze()
    o = sm.opening(plan, columns, evals, points, y, v, u_of)
    t.write_points([kv.commit(o["w"])])
    return plan, t.proof, o, (y, v)


def test_a_whole_stage_is_accepted_from_its_bytes_alone():
    plan, proof, o, (y, v) = proved()
    assert len(proof) == 32 * (4 + 9 + 2) and o["report"]["bad_sets"] == 0
    got, read = kv.verify_proof(proof, plan, K)
    assert got, got
    assert (read["challenges"]["y"], read["challenges"]["v"], read["challenges"]["u"]) == (y, v, o["u"]) and len(set(read["challenges"].values())) == 4
    assert len(read["points"]) == 6 and len(read["scalars"]) == 9 and all(mm.on_curve(p) and p is not None for p in read["points"])
    # one evaluation raised by 1 before it is written: the prover's report names the set, the verifier rejects the bytes
    plan, bad, o, _yv = proved(bump=(2, 1, 1))
    assert o["report"]["first_bad_set"] == 2 and kv.verify_proof(bad, plan, K)[0].reason == "equation"
    # one bit of an evaluation, of a commitment's sign, of [W]'s sign
    for byte in (32 * 4 + 5, 31, len(proof) - 1):
        bits = bytearray(proof)
        bits[byte] ^= 0x80 if byte % 32 == 31 else 1
        assert kv.verify_proof(bytes(bits), plan, K)[0].reason == "equation", byte
    for cut in (proof[:-1], proof + bytes(32)):
        with pytest.raises(ValueError):
            kv.verify_proof(cut, plan, K)
    with pytest.raises(ValueError):  # a scalar that is not below r
        kv.verify_proof(proof[:32 * 4] + R.to_bytes(32, "little") + proof[32 * 5:], plan, K)


def test_decompress_is_the_inverse_of_the_transcripts_compression():
    points = [None, G1, mm.neg(G1)] + [kv.fixed_mul(s) for s in nm.seeded_values(6, 0x6465)]
    assert {p[1] & 1 for p in points if p} == {0, 1}
    assert [kv.decompress(tm.point_compressed(p)) for p in points] == points
    with pytest.raises(ValueError):
        kv.decompress((4).to_bytes(32, "little"))  # 4^3 + 3 = 67 is no square mod q
    with pytest.raises(ValueError):
        kv.decompress(((mm.Q + 1) | 1 << 255).to_bytes(32, "little"))  # x = 1 again, written above q
    assert pow(67, (mm.Q - 1) // 2, mm.Q) == mm.Q - 1


# ---- the bases --------------------------------------------------------------------------------------------------------------------------

def test_tau_is_on_no_domain_and_the_bases_are_the_models_multiples():
    assert all(pow(TAU, 1 << k, R) != 1 for k in range(0, 29)) and 1 < TAU < R
    basis = kv.tau_basis(K, TAU)
    assert len(basis) == 1 << K and kv.tau_basis(K, TAU) is basis  # cached
    for i in (0, 1, 255, 256, 1023):
        assert basis[i] == mm.mul(pow(TAU, i, R), G1), i
    table = kv.byte_table()
    assert len(table) == 32 and all(len(row) == 255 for row in table) and table[0][0] == G1 and table[31][254] == mm.mul(255 << 248, G1)
    for s in (0, 1, 255, 256, R - 1, R, R + 5) + tuple(nm.seeded_values(3, 0x66786d)):
        assert kv.fixed_mul(s) == mm.mul(s, G1), s
    scalars, some = [0, 1, R - 1, R + 2] + nm.seeded_values(3, 0x6d736d), [G1, None, basis[1], basis[2], basis[3], basis[3], mm.neg(basis[3])]
    assert kv.msm(zip(scalars, some)) == mm.msm(scalars, some) and kv.msm([]) is None and kv.msm([(5, basis[7]), (R - 5, basis[7])]) is None
    lagrange, l_at = kv.lagrange_basis(K, TAU), kv.lagrange_at(K, TAU)
    for i in (0, 1, 513, 1023):
        assert lagrange[i] == mm.mul(l_at[i], G1), i
    assert sum(l_at) % R == 1 and sum(c * pow(nm.omega(K), i, R) for i, c in enumerate(l_at)) % R == TAU  # they interpolate 1 and X


def test_a_lagrange_commitment_of_cells_is_the_tau_commitment_of_their_coefficients():
    # the naive multi-scalar product on both sides at k = 4 ...
    cells = nm.seeded_values(16, 0x6c6167)
    coeff = nm.lagrange_to_coeff(cells, 4)
    assert [kv.evaluate(coeff, pow(nm.omega(4), i, R)) for i in range(16)] == cells
    assert mm.msm(cells, kv.lagrange_basis(4, TAU)) == mm.msm(coeff, kv.tau_basis(4, TAU)) == kv.commit(coeff)
    # ... at k = 10 over the rows of a column that is 0 but at three rows, and a seeded column by the exponents
    rows = {0: 5, 700: nm.seeded_values(1, 7)[0], 1023: R - 1}
    sparse = [rows.get(i, 0) for i in range(1 << K)]
    coeff = nm.lagrange_to_coeff(sparse, K)
    assert mm.msm(rows.values(), [kv.lagrange_basis(K, TAU)[i] for i in rows]) == kv.commit(coeff) and sum(1 for c in coeff if c) > 1000
    cells = nm.seeded_values(1 << K, 0x6c6168)
    assert sum(c * l for c, l in zip(cells, kv.lagrange_at(K, TAU))) % R == kv.evaluate(nm.lagrange_to_coeff(cells, K), TAU)


# ---- independence -----------------------------------------------------------------------------------------------------------------------

def test_the_verifier_imports_neither_the_prover_model_nor_the_product():
    tree = ast.parse((ROOT / "tests" / "kzg_verifier.py").read_text())
    imported = {a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names} | {node.module for node in ast.walk(tree) if isinstance(node, ast.ImportFrom)}
    assert imported == {"functools", "msm_model", "ntt_model", "transcript_model"}, imported
    assert not [w for w in ("__import__", "importlib", "import_module", "exec(", "ctypes") if w in (ROOT / "tests" / "kzg_verifier.py").read_text()]
