"""csrc/aesw_mont.h under csrc/aesw_fr.h and csrc/aesw_fq.h without a GPU: bn256's Fr and Fq in Montgomery form over one core,
compiled with g++ behind tests/field_driver.cpp and held against Python integers, each field to the same cases.  A value holds
v * 2^256 mod m; mont_mul(a, b) is a * b / 2^256 mod m on the integers, the field's inverse a^-1 * 2^512 and 0 for 0.  Every
ordered pair of the specials, the operands whose low limbs are all ones and 2 000 seeded values; the inverse once per value;
canonical flags on either side; the driver once more under AddressSanitizer and UBSan; Fr's byte table cell for cell."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
# limbs 0 ... 6 all 0xffffffff, the top limb as large as a canonical value of either field allows, and smaller ones
CARRIES = tuple((top << 224) | ((1 << 224) - 1) for top in (0x30644e71, 0x30644e70, 0x1fffffff, 1, 0))


class Field:
    def __init__(self, name, m, seed):
        self.name, self.m, self.seed = name, m, seed
        self.one = (1 << 256) % m  # the Montgomery form of 1
        self.r_inv = pow(1 << 256, -1, m)
        self.special = (0, 1, 2, m - 1, m - 2, 1 << 253, (m - 1) // 2, self.one, 3 * self.one % m)
        self.noncanonical = (m, m + 1, (1 << 256) - 1)

    def random(self, n=2000):
        rng = np.random.default_rng(self.seed)
        return [int.from_bytes(rng.bytes(40), "little") % self.m for _ in range(n)]


FR = Field("fr", 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001, 0x6672)
FQ = Field("fq", 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47, 0x6671)


def cells(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32)


def ints(block):
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(block, np.uint8).reshape(-1, 32)]


def build(tmp, flags=()):
    exe = tmp / ("field_driver" + ("_san" if flags else ""))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "field_driver.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def drive(exe, tmp, *args):
    out = subprocess.run([str(exe), *map(str, args), str(tmp / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return np.fromfile(tmp / "out.bin", np.uint8)


def run(exe, tmp, f, a, b):
    """(results: n x (mul, add, sub) x 32 bytes, flags) of the pairs (a[i], b[i]), both arrays of cells"""
    n = len(a)
    np.concatenate([a, b], axis=1).tofile(tmp / "in.bin")
    raw = drive(exe, tmp, f.name, tmp / "in.bin")
    assert raw.size == 97 * n
    return raw[:96 * n].reshape(n, 3, 32), raw[96 * n:]


def check(exe, tmp, f, a, b):
    """mul, add and sub of the pairs (a[i], b[i]) of integers are Python's.  The results are compared as bytes, all at once; only a
    difference is taken apart."""
    res, flags = run(exe, tmp, f, cells(a), cells(b))
    assert (flags == 3).all()
    m = f.m
    want = b"".join((x * y * f.r_inv % m).to_bytes(32, "little") + ((x + y) % m).to_bytes(32, "little") + ((x - y) % m).to_bytes(32, "little") for x, y in zip(a, b))
    if res.tobytes() != want:
        for x, y, (mul, add, sub) in zip(a, b, (ints(r) for r in res)):
            assert mul == x * y * f.r_inv % m, "%s: mont_mul(%#x, %#x) = %#x" % (f.name, x, y, mul)
            assert add == (x + y) % m, "%s: mont_add(%#x, %#x) = %#x" % (f.name, x, y, add)
            assert sub == (x - y) % m, "%s: mont_sub(%#x, %#x) = %#x" % (f.name, x, y, sub)
        raise AssertionError("the bytes differ and no value does")


def check_inverse(exe, tmp, f, values):
    cells(values).tofile(tmp / "inv.bin")
    got = ints(drive(exe, tmp, f.name, "--inv", tmp / "inv.bin"))
    assert len(got) == len(values)
    for x, i in zip(values, got):
        assert i == (pow(x, -1, f.m) * f.one * f.one % f.m if x else 0), "%s_inv(%#x) = %#x" % (f.name, x, i)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("field")


@pytest.fixture(scope="module")
def driver(tmp):
    return build(tmp)


@pytest.fixture(scope="module")
def sanitized(tmp):
    return build(tmp, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


@pytest.fixture(scope="module", params=(FR, FQ), ids=lambda f: f.name)
def field(request):
    return request.param


@pytest.fixture(scope="module")
def values(field):
    return list(field.special) + list(CARRIES) + field.random()


def test_the_core_is_free_of_hip_and_of_the_project_and_each_field_includes_it_alone():
    core = (CSRC / "aesw_mont.h").read_text()
    assert "hip/" not in core and "asm" not in core and '#include "' not in core
    for name, asserted in (("aesw_fr.h", ("FR_INV == 0xefffffffu", "FR_ONE", "FR_RAW_ONE", "fr_byte_table().cell[255]")),
                           ("aesw_fq.h", ("FQ_INV == 0xe4866389u", "FQ_ONE", "FQ_R2", "FQ_THREE"))):
        text = (CSRC / name).read_text()
        assert "hip/" not in text and "asm" not in text and re.findall(r'#include "([^"]*)"', text) == ["aesw_mont.h"], name
        for what in asserted:
            assert any(what in line for line in text.split("static_assert")[1:]), what
    # one product; a field's names for the core are references to its instantiations, never functions over it
    sources = [p for p in CSRC.rglob("*") if p.suffix in (".h", ".hip", ".cpp")]
    assert sum(len(re.findall(r"^AESW_\w+ constexpr \w+ \w*_mul\(", p.read_text(), re.M)) for p in sources) == 1
    assert "constexpr F mont_mul(const F &a, const F &b) {" in core
    for f, name in (("fr", "aesw_fr.h"), ("fq", "aesw_fq.h")):
        text = (CSRC / name).read_text()
        assert "inline constexpr auto &%s_mul = mont_mul<%s>;" % (f, f.capitalize()) in text
        assert re.findall(r"^AESW_\w+ constexpr \w+ (%s_\w+)\(" % f, text, re.M) == [f + "_inv"], name
    assert core.count("2 m < 2^255") == 1 and "< (1u << 30)" in core  # the bound on the modulus, once, for every field


def test_every_pair_against_python_integers(driver, tmp, field, values):
    f, n = field, len(values)
    assert n == 2014 and len(set(values)) == n and {f.one, 0, f.m - 1} <= set(values) and all(v < f.m for v in values)
    for v in CARRIES:
        assert cells([v])[0, :28].min() == 0xFF
    for first in range(0, n, 212):  # 10 runs of at most 212 x 2 014 pairs: every ordered pair once
        rows = values[first:first + 212]
        check(driver, tmp, f, [x for x in rows for _ in range(n)], values * len(rows))


def test_the_montgomery_form_of_one_is_the_identity(driver, tmp, field, values):
    res, _ = run(driver, tmp, field, cells(values), cells([field.one] * len(values)))
    assert ints(res[:, 0]) == values
    # the trait's constants are the field's
    assert ints(drive(driver, tmp, field.name, "--one")) == [field.one, 1]


def test_carries_run_through_every_limb(driver, tmp, field):
    m = field.m
    ops = list(CARRIES) + [m - 1, m - 2]
    check(driver, tmp, field, [x for x in ops for _ in ops], ops * len(ops))
    # the sums whose raw value passes 2^254, and the one that lands on m exactly
    check(driver, tmp, field, [m - 1, m - 1, (m + 1) // 2], [m - 1, 1, (m - 1) // 2])


def test_what_is_not_below_the_modulus_is_not_canonical(driver, tmp, field):
    m = field.m
    probes = list(field.noncanonical) + [m - 1, 0, m + (1 << 224), (m - 1) ^ (1 << 255)]
    _res, flags = run(driver, tmp, field, cells(probes), cells([0] * len(probes)))
    assert [int(f) & 1 for f in flags] == [0, 0, 0, 1, 1, 0, 0] and all(int(f) >> 1 == 1 for f in flags)
    _res, flags = run(driver, tmp, field, cells([0] * len(probes)), cells(probes))
    assert [int(f) >> 1 for f in flags] == [0, 0, 0, 1, 1, 0, 0] and all(int(f) & 1 == 1 for f in flags)


def test_the_inverse_of_every_value(driver, tmp, field, values):
    check_inverse(driver, tmp, field, values)  # once per value, not per pair


def test_the_byte_table_is_every_byte_value_in_montgomery_form(driver, tmp, pkg):
    want = b"".join(((v << 256) % FR.m).to_bytes(32, "little") for v in range(256))
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


def test_the_driver_runs_clean_under_address_and_ub_sanitizers(sanitized, tmp, field, values):
    first = len(field.special) + len(CARRIES)
    rows = values[:first + 32]
    check(sanitized, tmp, field, [x for x in rows for _ in rows], rows * len(rows))
    check_inverse(sanitized, tmp, field, rows)
    _res, flags = run(sanitized, tmp, field, cells(field.noncanonical), cells([1] * 3))
    assert [int(f) for f in flags] == [2, 2, 2]
