"""csrc/aesw_fq.h without a GPU: bn256's base field Fq in Montgomery form, compiled alone with g++ behind tests/fq_driver.cpp and
held against Python integers.  A coordinate holds v * 2^256 mod q; fq_mul(a, b) is a * b / 2^256 mod q on the integers, fq_add and
fq_sub their sum and difference mod q, fq_inv(a) the Montgomery form of the inverse (a^-1 * 2^512 on the integers) and 0 for 0.
Every ordered pair of {0, 1, q - 1, q - 2, 2, the Montgomery forms of 1 and of 3, operands whose low limbs are all 0xffffffff,
100 seeded values}; q, q + 1 and 2^256 - 1 are not canonical; the same driver once more under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
MONT = (1 << 256) % Q
MONT_INV = pow(MONT, -1, Q)
SPECIAL = (0, 1, Q - 1, Q - 2, 2, MONT, 3 * MONT % Q)
CARRIES = tuple((top << 224) | ((1 << 224) - 1) for top in (0x30644e71, 0x1fffffff, 0))
NONCANONICAL = (Q, Q + 1, (1 << 256) - 1)


def cells(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32)


def ints(block):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(block, np.uint8).reshape(-1, 32)]


def build(tmp, flags=()):
    exe = tmp / ("fq_driver" + ("_san" if flags else ""))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "fq_driver.cpp"), "-o", str(exe)], check=True)
    return exe


def run(exe, tmp, a, b):
    """(mul, add, sub, inv of a, flags) of the pairs (a[i], b[i])"""
    n = len(a)
    np.concatenate([cells(a), cells(b)], axis=1).tofile(tmp / "in.bin")
    out = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(tmp / "out.bin", np.uint8)
    assert raw.size == 129 * n
    res = raw[:128 * n].reshape(n, 4, 32)
    return [ints(res[:, i]) for i in range(4)] + [raw[128 * n:]]


def check(exe, tmp, a, b):
    mul, add, sub, inv, flags = run(exe, tmp, a, b)
    assert (flags == 3).all()
    for x, y, m, s, d, i in zip(a, b, mul, add, sub, inv):
        assert m == x * y * MONT_INV % Q, "fq_mul(%#x, %#x) = %#x" % (x, y, m)
        assert s == (x + y) % Q, "fq_add(%#x, %#x) = %#x" % (x, y, s)
        assert d == (x - y) % Q, "fq_sub(%#x, %#x) = %#x" % (x, y, d)
        assert i == (pow(x, -1, Q) * MONT * MONT % Q if x else 0), "fq_inv(%#x) = %#x" % (x, i)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fq")


@pytest.fixture(scope="module")
def values():
    rng = np.random.default_rng(0x6671)
    return list(SPECIAL) + list(CARRIES) + [int.from_bytes(rng.bytes(40), "little") % Q for _ in range(100)]


def test_the_header_is_free_of_hip_and_of_the_project():
    text = (ROOT / "halo2-aes_amd" / "csrc" / "aesw_fq.h").read_text()
    assert "hip/" not in text and "asm" not in text and '#include "' not in text
    for asserted in ("FQ_INV == 0xe4866389u", "FQ_ONE", "FQ_R2", "FQ_THREE"):
        assert any(asserted in line for line in text.split("static_assert")[1:]), asserted


def test_every_pair_against_python_integers(tmp, values):
    exe = build(tmp)
    for v in CARRIES:
        assert v < Q and cells([v])[0, :28].min() == 0xFF
    check(exe, tmp, [x for x in values for _ in values], values * len(values))
    mul = run(exe, tmp, values, [MONT] * len(values))[0]
    assert mul == values  # the Montgomery form of 1 is the identity


def test_what_is_not_below_q_is_not_canonical(tmp):
    exe = build(tmp)
    probes = list(NONCANONICAL) + [Q - 1, 0, Q + (1 << 224), (Q - 1) ^ (1 << 255)]
    flags = run(exe, tmp, probes, [0] * len(probes))[-1]
    assert [int(f) & 1 for f in flags] == [0, 0, 0, 1, 1, 0, 0] and all(int(f) >> 1 == 1 for f in flags)


def test_the_driver_runs_clean_under_address_and_ub_sanitizers(tmp, values):
    exe = build(tmp, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rows = values[:24]
    check(exe, tmp, [x for x in rows for _ in rows], rows * len(rows))
