"""The one build table of the libraries next to libaesw.so (_build.LIBRARIES) without a GPU: its names and their order, every
entry's sources and headers, that api._LIBRARIES follows it, and that build() builds and loads exactly its entries."""
import pytest

import check_library as cl

NAMES = ["circ", "cols", "vals", "acc", "perm", "vacc", "mult", "theta", "grand", "sigma", "ntt", "quot", "open"]
# what an entry depends on beyond SATELLITE_HEADERS, by file name and in the table's order
HEADERS = {
    "circ": ["aesw_circ_search.h"],
    "cols": ["aesw_circ_search.h", "aesw_fr.h"],
    "vals": ["aesw_vals_check.h"],
    "acc": ["aesw_mult.h", "aesw_mult_dev.h", "aesw_run.h", "aesw_mult.h"],
    "perm": ["aesw_mult.h", "aesw_perm.h", "aesw_mult.h"],
    "vacc": ["aesw_mult.h", "aesw_mult_dev.h", "aesw_run.h", "aesw_vals_check.h", "aesw_vacc.h", "aesw_mult.h"],
    "mult": ["aesw_mult.h", "aesw_mult_dev.h"],
    "theta": ["aesw_fr.h", "aesw_theta.h", "aesw_mult.h", "aesw_mult.h"],
    "grand": ["aesw_fr.h", "aesw_grand.h", "aesw_theta.h", "aesw_mult.h", "aesw_mult.h"],
    "sigma": ["aesw_fr.h", "aesw_sigma.h"],
    "ntt": ["aesw_fr.h", "aesw_sigma.h", "aesw_ntt.h"],
    "quot": ["aesw_fr.h", "aesw_sigma.h", "aesw_ntt.h", "aesw_theta.h", "aesw_placement.h", "aesw_quot.h"],
    "open": ["aesw_fr.h", "aesw_open.h"],
}
GONE = ("SATELLITES", "FIELD_LIBRARIES", "ARGUMENT_LIBRARIES", "DOMAIN_LIBRARIES", "QUOTIENT_LIBRARIES", "OPENING_LIBRARIES",
        "domain_library_names", "quotient_library_names", "opening_library_names")


def test_the_table_names_the_thirteen_in_build_order():
    b = cl.build_module()
    assert b.library_names() == NAMES == list(b.LIBRARIES)
    with pytest.raises(KeyError):
        b.library_entry("nowhere")
    assert not [name for name in GONE if hasattr(b, name)]
    assert not [name for name in vars(b) if name.endswith("_LIB") and name != "HOST_LIB"]  # the per-library path constants went with them


@pytest.mark.parametrize("name", NAMES)
def test_an_entry_is_its_sources_its_headers_and_its_public_header(name):
    b = cl.build_module()
    sources, headers, public = b.library_entry(name)
    assert sources and all(s.exists() and s.parent == b.CSRC / name and s.suffix == ".hip" for s in sources), sources
    assert public == b.INCLUDE / ("aesw_%s.h" % name) and public.exists()
    assert [h.name for h in headers] == HEADERS[name] and all(h.exists() and h.parent in (b.CSRC, b.INCLUDE) for h in headers)


def test_the_loader_lists_the_table_in_its_order(pkg):
    assert list(pkg.api._LIBRARIES) == ["aesw", "host"] + cl.build_module().library_names()
    for name in NAMES:
        path, _symbols, hint = pkg.api._LIBRARIES[name]
        assert path == getattr(pkg.api, name.upper() + "_LIB_PATH") == pkg.api.LIB_PATH.parent / ("libaesw_%s.so" % name) and hint == pkg.api._NO_FALLBACK


def test_build_builds_and_loads_exactly_the_table(pkg, monkeypatch):
    import __graft_entry__ as ge
    built, loaded, b = [], [], cl.build_module()
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    for name in NAMES:
        monkeypatch.setattr(pkg.api, "load_%s_library" % name, lambda path=None, name=name: loaded.append(name))
    ge.build()  # everything else is built already (the pkg fixture), so the rest of it finds nothing to do
    assert built == NAMES == loaded
