"""The argument rules the libraries next to libaesw.so share (csrc/aesw_entry_rules.h: the DENSE-or-PACKED layout, the bounds of
k and n_sets, "there and aligned" for a report and for the block slabs, when the key columns count, and what both accumulators
check of their outputs; the challenges, the outputs and the workspace of the grand-product calls).  The header is compiled alone with g++ -- no ROCm include, no context, no GPU -- behind
tests/entry_rules_driver.cpp.  Every text is held against MESSAGES, written out here as the entry points said them before the
rules were stated once; for each rule the smallest accepting argument and the nearest refusing one."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MESSAGES = {
    "layout": "the layout must be DENSE or PACKED (a VALUES witness has no x)",
    "k": "k must be 2 ... 30",
    "sets": "n_sets must be 1 ... 1024",
    "report": "d_report must be there and 8-byte aligned",
    "slabs": "d_x, d_y and d_z must be there and 16-byte aligned",
    "keys": "the key columns must be 16-byte aligned",
    "mult": "d_mult must be there and 16-byte aligned",
    "challenges": "d_beta and d_gamma must be there and 16-byte aligned",
    "product_outputs": "d_z_fr and d_closing_fr must be there and 16-byte aligned",
    "workspace": "d_workspace must be there and 16-byte aligned",
}
OK = "-"
A = 0x10000  # an address aligned to anything asked here
DENSE, PACKED, VALUES = 0, 1, 2
FIRST_K_WITH_KEY_ROWS = 9  # 2^9 = 512 >= 400 rows of the key schedule


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("entry_rules") / "entry_rules_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "entry_rules_driver.cpp"), "-o", str(exe)], check=True)

    def ask(*commands):
        text = "\n".join(" ".join(str(v) for v in c) for c in commands)
        done = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        out = done.stdout.splitlines()
        assert len(out) == len(commands), (done.stdout, done.stderr)
        return out
    return ask


def test_the_header_needs_neither_rocm_nor_the_context():
    for name in ("aesw_entry_rules.h", "aesw_align.h"):
        text = (ROOT / "halo2-aes_amd" / "csrc" / name).read_text()
        includes = [line for line in text.splitlines() if line.startswith("#include")]
        assert includes and not [line for line in includes if "hip" in line or "aesw_ctx" in line or "aesw_entry.h" in line], includes


def test_the_layout_is_dense_or_packed(ask):
    assert ask(("layout", DENSE), ("layout", PACKED), ("layout", VALUES), ("layout", 3), ("layout", -1)) == \
        [OK, OK, MESSAGES["layout"], MESSAGES["layout"], MESSAGES["layout"]]


def test_the_bounds_of_k_and_of_the_sets(ask):
    assert ask(("k", 1), ("k", 2), ("k", 30), ("k", 31), ("k", 0)) == [MESSAGES["k"], OK, OK, MESSAGES["k"], MESSAGES["k"]]
    assert ask(("sets", 0), ("sets", 1), ("sets", 1024), ("sets", 1025)) == [MESSAGES["sets"], OK, OK, MESSAGES["sets"]]


def test_a_report_is_there_and_eight_byte_aligned(ask):
    assert ask(("report", A), ("report", A + 8), ("report", A + 4), ("report", A + 1), ("report", 0)) == \
        [OK, OK, MESSAGES["report"], MESSAGES["report"], MESSAGES["report"]]


def test_the_slabs_are_there_and_sixteen_byte_aligned(ask):
    bad = MESSAGES["slabs"]
    assert ask(("slabs", A, A + 16, A + 32)) == [OK]
    # a pointer off by 8 where 16 is asked, each column in turn; then each column missing
    assert ask(("slabs", A + 8, A, A), ("slabs", A, A + 8, A), ("slabs", A, A, A + 8)) == [bad] * 3
    assert ask(("slabs", 0, A, A), ("slabs", A, 0, A), ("slabs", A, A, 0)) == [bad] * 3


def test_when_the_key_columns_count_and_when_they_are_refused(ask):
    k = FIRST_K_WITH_KEY_ROWS
    assert ask(("keys", k, 1, A, A + 16, A + 32)) == ["1 " + OK]
    # no slab, or one column missing: no key lookups and no refusal -- not even where another column is misaligned
    assert ask(("keys", k, 0, A, A, A), ("keys", k, 1, 0, A, A), ("keys", k, 1, A, 0, A), ("keys", k, 1, A, A, 0), ("keys", k, 1, A + 8, A, 0)) == ["0 " + OK] * 5
    # one column misaligned: a refusal
    assert ask(("keys", k, 1, A + 8, A, A), ("keys", k, 1, A, A + 8, A), ("keys", k, 1, A, A, A + 8)) == ["1 " + MESSAGES["keys"]] * 3
    # k below the first k with key rows: the circuit has no key selector, the columns do not count and are not looked at
    assert ask(("keys", k - 1, 1, A, A, A), ("keys", k - 1, 1, A + 8, A + 4, A + 1), ("keys", 2, 1, A, A, A)) == ["0 " + OK] * 3
    assert ask(("keys", 30, 1, A, A, A)) == ["1 " + OK]


def test_what_the_accumulators_check_of_their_outputs_in_their_order(ask):
    assert ask(("outputs", 2, 1, 1, A, A), ("outputs", 30, 1, 1024, A + 16, A + 8)) == [OK, OK]
    # k first, then the sets, then the report, then d_mult
    assert ask(("outputs", 1, 1, 0, 0, 0), ("outputs", 31, 1, 1, A, A)) == [MESSAGES["k"]] * 2
    assert ask(("outputs", 2, 1, 0, 0, 0), ("outputs", 2, 1, 1025, A, A)) == [MESSAGES["sets"]] * 2
    assert ask(("outputs", 2, 1, 1, 0, 0), ("outputs", 2, 1, 1, A + 8, A + 4)) == [MESSAGES["report"]] * 2
    assert ask(("outputs", 2, 1, 1, 0, A), ("outputs", 2, 1, 1, A + 8, A)) == [MESSAGES["mult"]] * 2
    # a call that takes no k (the reset) does not look at it
    assert ask(("outputs", 0, 0, 1, A, A), ("outputs", 99, 0, 0, A, A)) == [OK, MESSAGES["sets"]]


def test_what_the_grand_product_calls_take_alike(ask):
    for rule in ("challenges", "product_outputs"):  # a pair of Fr cells or columns: both there, both 16-byte aligned
        bad = MESSAGES[rule]
        assert ask((rule, A, A + 32), (rule, A + 16, A)) == [OK, OK]
        assert ask((rule, 0, 0), (rule, 0, A), (rule, A, 0)) == [bad] * 3
        assert ask((rule, A + 8, A + 8), (rule, A + 8, A), (rule, A, A + 8), (rule, A + 1, A), (rule, A, A + 4)) == [bad] * 5
    bad = MESSAGES["workspace"]
    assert ask(("workspace", A), ("workspace", A + 16)) == [OK, OK]
    assert ask(("workspace", 0), ("workspace", A + 8), ("workspace", A + 4), ("workspace", A + 1)) == [bad] * 4
