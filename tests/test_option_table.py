"""The one table of options (csrc/aesw_options.h) against the options as they have always been (tests/option_table.py EXPECTED,
written from the two strcmp chains the table replaced).  The header is compiled alone with g++ -- no ROCm include, no GPU -- into
tests/option_table_driver.cpp, which dumps the rows and drives set / get through the table's own functions:

  * the rows are exactly the expected names, each with its default, lowest and highest accepted value, form, and whether it can be
    set and read;
  * every settable row takes its lowest and highest value and reads them back; one below and one above are refused and leave the
    value as it was; names that share a field read each other's writes; a read-only name refuses every set;
  * the prose in front of aesw_set_option in include/aesw.h quotes every name that is not build-only, and no name the table lacks."""
import re

import pytest

import option_table as ot


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ot.build_driver(tmp_path_factory.mktemp("option_table"))


def test_rows_are_what_the_library_always_accepted(driver):
    rows = ot.dump(driver)
    assert sorted(rows) == sorted(ot.EXPECTED)
    assert {n for n, (_r, build_only) in rows.items() if build_only} == ot.BUILD_ONLY
    assert {n for n, (r, _b) in rows.items() if r.default is None} == ot.FIELDLESS
    for name, exp in ot.EXPECTED.items():
        got = rows[name][0]
        assert (got.settable, got.readable, got.form) == (exp.settable, exp.readable, exp.form), name
        if exp.settable or name in ot.BUILD_ONLY:
            assert (got.lo, got.hi) == (exp.lo, exp.hi), name
        if got.default is not None:
            assert got.default == exp.default, name


def test_set_and_get_through_the_table(driver):
    for name, row in ot.EXPECTED.items():
        if not row.settable:
            assert ot.drive(driver, [("s", name, 0), ("s", name, 1)]) == [None, None], name  # read-only (or not in this build)
            continue
        has_field = name not in ot.FIELDLESS
        for v in ot.inside(row):
            stored = (1 if v else 0) if row.form == "truthy" else v
            got = ot.drive(driver, [("s", name, v), ("g", name)])
            assert got == [True, stored if has_field else None], (name, v)  # a row without a field: the library's follow-up stores
        for v in ot.outside(row):
            keep = ot.inside(row)[0]
            got = ot.drive(driver, [("s", name, keep), ("s", name, v), ("g", name)])
            assert got == [True, None, keep if has_field else None], (name, v)
    assert ot.drive(driver, [("s", "no_such_option", 0), ("g", "no_such_option")]) == [None, None]


def test_defaults_read_through_the_table(driver):
    for name, row in ot.EXPECTED.items():
        if name not in ot.FIELDLESS:
            assert ot.drive(driver, [("g", name)]) == [row.default], name


def test_aliases_read_each_others_writes(driver):
    assert ot.ALIASES == (("nt_stores", "store_mode"),)
    d = lambda script: ot.drive(driver, script)  # noqa: E731
    assert d([("s", "store_mode", 2), ("g", "nt_stores"), ("g", "store_mode")]) == [True, 0, 2]  # write-through is not "nontemporal"
    assert d([("s", "store_mode", 1), ("g", "nt_stores")]) == [True, 1]
    assert d([("s", "store_mode", 0), ("g", "nt_stores")]) == [True, 0]
    assert d([("s", "store_mode", 2), ("s", "nt_stores", 7), ("g", "store_mode"), ("g", "nt_stores")]) == [True, True, 1, 1]
    assert d([("s", "nt_stores", 0), ("g", "store_mode")]) == [True, 0]
    # every other pair of names has a field of its own
    every = [n for n in ot.EXPECTED if n not in ot.FIELDLESS and n not in ot.ALIASES[0]]
    script = [("s", n, ot.EXPECTED[n].hi) for n in every] + [("g", n) for n in every]
    assert d(script) == [True] * len(every) + [ot.EXPECTED[n].hi for n in every]


def test_the_prose_of_aesw_h_names_the_same_options(driver):
    rows = ot.dump(driver)
    text = (ot.ROOT / "include" / "aesw.h").read_text()
    comment = text[text.index("/* ---- tuning / introspection"):text.index("int aesw_set_option(")]
    quoted = set(re.findall(r'"([a-z0-9_]+)"', comment))
    documented = {n for n, (_r, build_only) in rows.items() if not build_only}
    assert documented - quoted == set(), "options the comment in front of aesw_set_option does not name"
    assert quoted - set(rows) == set(), "names the comment quotes that are no options"
