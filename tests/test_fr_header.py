"""csrc/aesw_fr.h without a GPU: bn256's Fr in Montgomery form, compiled alone with g++ behind tests/fr_driver.cpp and held
against Python integers.  A cell holds v * 2^256 mod r; fr_mul(a, b) is a * b / 2^256 mod r on the cells' integers, fr_add their
sum mod r.  Every pair of {0, 1, 2, r - 1, r - 2, 2^253, (r - 1) / 2, the Montgomery form of 1, 2 000 seeded random canonical
values}; operands whose limbs are all 0xffffffff below the top, so that every carry runs; r, r + 1 and 2^256 - 1 are not
canonical; the same driver once more as a stand-alone program under AddressSanitizer and UBSan.  The byte table
(fr_byte_table: cell v = v * 2^256 mod r) cell for cell, and through the built columns checker, which fills its table from it."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
R_INV = pow(1 << 256, -1, R)
SPECIAL = (0, 1, 2, R - 1, R - 2, 1 << 253, (R - 1) // 2, (1 << 256) % R)
# limbs 0 ... 6 all 0xffffffff, the top limb as large as a canonical value allows, and smaller ones
CARRIES = tuple((top << 224) | ((1 << 224) - 1) for top in (0x30644e71, 0x30644e70, 0x1fffffff, 1, 0))
NONCANONICAL = (R, R + 1, (1 << 256) - 1)


def cells(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32)


def ints(block):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(block, np.uint8).reshape(-1, 32)]


def build(tmp, flags=()):
    exe = tmp / ("fr_driver" + ("_san" if flags else ""))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "fr_driver.cpp"), "-o", str(exe)], check=True)
    return exe


def run(exe, tmp, a, b):
    """(mul, add, flags) of the pairs (a[i], b[i])"""
    n = len(a)
    np.concatenate([cells(a), cells(b)], axis=1).tofile(tmp / "in.bin")
    out = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = np.fromfile(tmp / "out.bin", np.uint8)
    assert raw.size == 65 * n
    res = raw[:64 * n].reshape(n, 2, 32)
    return ints(res[:, 0]), ints(res[:, 1]), raw[64 * n:]


def check(exe, tmp, a, b):
    mul, add, flags = run(exe, tmp, a, b)
    assert (flags == 3).all()
    for x, y, m, s in zip(a, b, mul, add):
        assert m == x * y * R_INV % R, "fr_mul(%#x, %#x) = %#x" % (x, y, m)
        assert s == (x + y) % R, "fr_add(%#x, %#x) = %#x" % (x, y, s)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fr")


@pytest.fixture(scope="module")
def driver(tmp):
    return build(tmp)


@pytest.fixture(scope="module")
def values():
    rng = np.random.default_rng(0x6672)
    return list(SPECIAL) + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(2000)]


def test_every_pair_against_python_integers(driver, tmp, values):
    assert (1 << 256) % R in values and len(values) == 2008
    n = len(values)
    for first in range(0, n, 251):  # 8 runs of 251 x 2 008 pairs: every ordered pair once
        rows = values[first:first + 251]
        check(driver, tmp, [x for x in rows for _ in range(n)], values * len(rows))


def test_the_montgomery_form_of_one_is_the_identity(driver, tmp, values):
    one = (1 << 256) % R
    mul, _add, _ = run(driver, tmp, values, [one] * len(values))
    assert mul == values


def test_carries_run_through_every_limb(driver, tmp):
    for v in CARRIES:
        assert v < R and cells([v])[0, :28].min() == 0xFF
    ops = list(CARRIES) + [R - 1, R - 2]
    check(driver, tmp, [x for x in ops for _ in ops], ops * len(ops))
    # the sums whose raw value passes 2^254, and the one that lands on r exactly
    check(driver, tmp, [R - 1, R - 1, (R + 1) // 2], [R - 1, 1, (R - 1) // 2])


def test_what_is_not_below_r_is_not_canonical(driver, tmp):
    probes = list(NONCANONICAL) + [R - 1, 0, R + (1 << 224), (R - 1) ^ (1 << 255)]
    _mul, _add, flags = run(driver, tmp, probes, [0] * len(probes))
    assert [int(f) & 1 for f in flags] == [0, 0, 0, 1, 1, 0, 0] and all(int(f) >> 1 == 1 for f in flags)
    _mul, _add, flags = run(driver, tmp, [0] * len(probes), probes)
    assert [int(f) >> 1 for f in flags] == [0, 0, 0, 1, 1, 0, 0]


def test_the_byte_table_is_every_byte_value_in_montgomery_form(driver, tmp, pkg):
    want = b"".join(((v << 256) % R).to_bytes(32, "little") for v in range(256))
    subprocess.run([str(driver), "--byte-table", str(tmp / "table.bin")], check=True)
    got = (tmp / "table.bin").read_bytes()
    assert len(got) == 256 * 32
    for v in range(256):
        assert got[32 * v:32 * v + 32] == want[32 * v:32 * v + 32], v
    # the built library fills its table from the header: the same bytes, and the hash the search found over them before
    lib = pkg.api.load_cols_library()
    table, inv = (ctypes.c_uint8 * 8192)(), (ctypes.c_uint8 * 4096)()
    lib.aesw_cols_fr_table(table)
    assert bytes(table) == want
    mul, bits = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.aesw_cols_hash_search(table, ctypes.byref(mul), ctypes.byref(bits), inv) == 0
    assert (mul.value, bits.value) == (0x309119E3, 8)  # read once from the library as it was built with its own U256 copy
    assert sorted(inv[((int.from_bytes(want[32 * v:32 * v + 4], "little") * mul.value) & 0xFFFFFFFF) >> (32 - bits.value)] for v in range(256)) == list(range(256))


def test_the_driver_runs_clean_under_address_and_ub_sanitizers(tmp, values):
    exe = build(tmp, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rows = (list(SPECIAL) + list(CARRIES) + values[8:40])
    check(exe, tmp, [x for x in rows for _ in rows], rows * len(rows))
    _m, _a, flags = run(exe, tmp, list(NONCANONICAL), [1] * 3)
    assert [int(f) for f in flags] == [2, 2, 2]
