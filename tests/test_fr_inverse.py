"""csrc/aesw_fr.h's inverse without a GPU: fr_inv, fr_is_zero and fr_eq (the core's, under Fr's names) compiled alone with g++
behind tests/fr_inv_driver.cpp and held against tests/grand_model.py (pow(x, r - 2, r), 0 for 0) over Fr's value set of
tests/test_field_headers.py -- 0, 1, r - 1 and the Montgomery form of 1 among them, the operands whose limbs are all 0xffffffff
below the top, 2 000 seeded random canonical values.  A cell holds v * 2^256 mod r, so the inverse CELL of a cell x is
x^-1 * 2^512 mod r and fr_mul(fr_inv(x), x) is the cell of 1.  The same driver once more as a stand-alone program under
AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grand_model as gm
import test_field_headers as fh

ROOT = Path(__file__).resolve().parent.parent
ONE = (1 << 256) % gm.R


def build(tmp, flags=()):
    exe = tmp / ("fr_inv_driver" + ("_san" if flags else ""))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "fr_inv_driver.cpp"), "-o", str(exe)], check=True)
    return exe


def check(exe, tmp, cells_in):
    """every cell's inverse is the model's and multiplies back to one"""
    n = len(cells_in)
    fh.cells(cells_in).tofile(tmp / "inv_in.bin")
    out = subprocess.run([str(exe), str(tmp / "inv_in.bin"), str(tmp / "inv_out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(tmp / "inv_out.bin", np.uint8)
    assert raw.size == 65 * n
    res, flags = raw[:64 * n].reshape(n, 2, 32), raw[64 * n:]
    inverse, back = fh.ints(res[:, 0]), fh.ints(res[:, 1])
    for x, i, b, f in zip(cells_in, inverse, back, flags):
        residue = x * gm.M_INV % gm.R
        assert i == gm.inv(residue) * gm.M % gm.R, "fr_inv(%#x) = %#x" % (x, i)
        assert i == pow(residue, gm.R - 2, gm.R) * gm.M % gm.R  # the model's memo is the definition
        assert b == (ONE if x else 0), "fr_inv(%#x) * itself = %#x" % (x, b)
        assert int(f) == (1 if x == 0 else 0) | 2 | (4 if x == ONE else 0) | (8 if x == i else 0), (hex(x), int(f))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fr_inv")


@pytest.fixture(scope="module")
def values():
    assert fh.FR.m == gm.R
    return list(fh.FR.special) + fh.FR.random()  # the values of tests/test_field_headers.py


def test_the_inverse_is_the_models_and_multiplies_back_to_one(tmp, values):
    assert {0, 1, gm.R - 1, ONE} <= set(values) and len(values) == 2009
    check(build(tmp), tmp, values + list(fh.CARRIES))


def test_zero_inverts_to_zero_and_the_self_inverse_cells_are_one_and_minus_one(tmp):
    exe = build(tmp)
    fh.cells([0, ONE, gm.R - ONE, 2]).tofile(tmp / "few.bin")
    subprocess.run([str(exe), str(tmp / "few.bin"), str(tmp / "few_out.bin")], check=True)
    raw = np.fromfile(tmp / "few_out.bin", np.uint8)
    inverse = fh.ints(raw[:256].reshape(4, 2, 32)[:, 0])
    assert inverse[:3] == [0, ONE, gm.R - ONE] and [int(f) for f in raw[256:]] == [1 | 2 | 8, 2 | 4 | 8, 2 | 8, 2]


def test_the_driver_runs_clean_under_address_and_ub_sanitizers(tmp, values):
    exe = build(tmp, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check(exe, tmp, list(fh.FR.special) + list(fh.CARRIES) + values[9:73])
