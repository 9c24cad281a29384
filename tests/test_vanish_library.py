"""libaesw_vanish.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_vanish_ functions include/aesw_vanish.h declares, api.VANISH_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * it is the entry of the fifth build table, _build.VANISHING_LIBRARIES, and of api._VANISHING_LIBRARIES -- not of the first four,
    which stay what their tests pin -- and build() builds it through build_vanishing, last, and loads it;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/vanish_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic, the field products as 64-bit multiply-adds, at most 256 unified
    registers, one cell stored per lane (a rotated cell comes through the cache, the faster of the two measured,
    profiles/vanish/README.md; the table records it, no assertion pins it); compared with the tracked table profiles/isa_resources_vanish.json
    (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_vanish_library.py);
  * the other libraries carry none of the new symbols, and the header names no other library."""
import subprocess

import check_library as cl
import vanish_cases as vc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_vanish.json"
code_object = cl.code_object_fixture("VANISH_LIB_PATH")
DECLARED = ["aesw_vanish_divide_device", "aesw_vanish_head_device", "aesw_vanish_lookup_device", "aesw_vanish_perm_device", "aesw_vanish_scalars_bytes",
            "aesw_vanish_scalars_device", "aesw_vanish_scalars_offset", "aesw_vanish_shape_ok", "aesw_vanish_tables_bytes", "aesw_vanish_tables_device"]
METHODS = ("vanishing_tables", "vanishing_scalars", "vanishing_scalar", "quotient_accumulator", "quotient_extended")


def other_tables(b, api):
    return (b.LIBRARIES, b.CURVE_LIBRARIES, b.PROOF_LIBRARIES, b.MULTIOPEN_LIBRARIES, api._LIBRARIES, api._CURVE_LIBRARIES, api._PROOF_LIBRARIES, api._MULTIOPEN_LIBRARIES)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.VANISH_LIB_PATH
    assert lib.name == "libaesw_vanish.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    assert cl.declared("aesw_vanish.h", "aesw_vanish_") == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == DECLARED, sorted(exported)[:20]
    loaded = api.load_vanish_library()
    assert api.load_vanish_library() is loaded and sorted(api.VANISH_SYMBOLS) == DECLARED and all(getattr(loaded, f) is not None for f in DECLARED)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = cl.build_module()
    others = b.library_names() + b.curve_library_names() + b.proof_library_names() + b.multiopen_library_names()
    assert not [n for n in others + ["host"] if "libaesw_%s" % n in dyn], dyn
    source = (cl.ROOT / "halo2-aes_amd" / "csrc" / "vanish" / "aesw_vanish.hip").read_text()
    assert "namespace aesw_vanish {" in source and all('#include "../%s"' % h in source for h in ("aesw_fr_dev.h", "aesw_quot.h", "aesw_vanish.h"))
    header = (cl.ROOT / "include" / "aesw_vanish.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1 and "NOT PINNED" in header
    assert not [n for n in others if "aesw_" + n in header]
    assert len(api.VANISH_TABLES) == 9 and all("AESW_VANISH_%s %du" % (name.upper(), i) in header for i, name in enumerate(api.VANISH_TABLES))


def test_the_fifth_table_has_the_shape_of_the_first_and_build_walks_it_last(pkg, monkeypatch):
    import __graft_entry__ as ge
    b, api = cl.build_module(), pkg.api
    assert b.vanishing_library_names() == ["vanish"] == list(b.VANISHING_LIBRARIES) == list(api._VANISHING_LIBRARIES)
    assert not [t for t in other_tables(b, api) if "vanish" in t]
    # the first four tables stay what their tests pin
    assert len(b.LIBRARIES) == 13 and len(api._LIBRARIES) == 15 and list(b.CURVE_LIBRARIES) == ["msm"] == list(api._CURVE_LIBRARIES)
    assert list(b.PROOF_LIBRARIES) == ["transcript"] == list(api._PROOF_LIBRARIES) and list(b.MULTIOPEN_LIBRARIES) == ["shplonk"] == list(api._MULTIOPEN_LIBRARIES)
    sources, headers, public = b.VANISHING_LIBRARIES["vanish"]
    assert sources and all(s.exists() and s.parent == b.CSRC / "vanish" and s.suffix == ".hip" for s in sources)
    assert [h.name for h in headers] == ["aesw_fr.h", "aesw_sigma.h", "aesw_ntt.h", "aesw_theta.h", "aesw_quot.h", "aesw_vanish.h"]
    assert all(h.exists() and h.parent == b.CSRC for h in headers)
    assert public == b.INCLUDE / "aesw_vanish.h" and public.exists()
    assert api._VANISHING_LIBRARIES["vanish"] == (api.VANISH_LIB_PATH, api.VANISH_SYMBOLS, api._NO_FALLBACK)
    built, loaded = [], []
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    monkeypatch.setattr(b, "build_curve", lambda name, force=False: built.append("curve:" + name))
    monkeypatch.setattr(b, "build_proof", lambda name, force=False: built.append("proof:" + name))
    monkeypatch.setattr(b, "build_multiopen", lambda name, force=False: built.append("multiopen:" + name))
    monkeypatch.setattr(b, "build_vanishing", lambda name, force=False: built.append("vanishing:" + name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    for name in ("shplonk", "vanish"):
        monkeypatch.setattr(api, "load_%s_library" % name, lambda path=None, name=name: loaded.append(name))
    ge.build()
    assert built == b.library_names() + ["curve:msm", "proof:transcript", "multiopen:shplonk", "vanishing:vanish"] and loaded == ["shplonk", "vanish"]


def test_the_shape_query_is_the_headers_bounds(pkg):
    ok = pkg.api.load_vanish_library().aesw_vanish_shape_ok
    assert ok(10, 12, 1, 1, 3, 1018) and ok(10, 12, 0, 1024, 1, 1) and ok(26, 28, 1, 4, 3, (1 << 26) - 1) and ok(10, 14, 1, 1, 8, 1023)
    for bad in ((9, 12, 1, 1, 3, 100), (10, 11, 1, 1, 3, 100), (27, 29, 1, 1, 3, 100), (10, 12, 2, 1, 3, 100), (10, 12, 1, 0, 3, 100), (10, 12, 1, 1025, 3, 100),
                (10, 12, 1, 1, 0, 100), (10, 12, 1, 1, 4, 100), (10, 13, 1, 1, 8, 100), (10, 14, 1, 1, 9, 100), (10, 12, 1, 1, 3, 0), (10, 12, 1, 1, 3, 1024)):
        assert not ok(*bad), bad  # tests/test_quot_model.py's list for quot_shape_ok


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "vanish", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    others = dict(pkg.api._LIBRARIES, **pkg.api._CURVE_LIBRARIES, **pkg.api._PROOF_LIBRARIES, **pkg.api._MULTIOPEN_LIBRARIES)
    for other, (path, _symbols, _hint) in others.items():
        text = cl.nm(path, "-C")
        assert not [w for w in ("aesw_vanish", "vanish_head_kernel", "vanish_perm_kernel", "vanish_lookup_kernel", "vanish_divide_kernel") if w in text], other
    naming = sorted(h.name for h in (cl.ROOT / "include").glob("*.h") if h.name != "aesw_vanish.h" and "aesw_vanish" in h.read_text())
    assert naming == []


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_the_accumulator_refuses_a_segment_out_of_order_before_it_calls(pkg):
    """_turn needs no device: the order is the accumulator's own"""
    api = pkg.api
    acc = api.QuotientAccumulator.__new__(api.QuotientAccumulator)
    acc._order = [("head", 0), ("permutation_set", 0), ("permutation_set", 1), ("lookup_set", 0), ("divide", 0)]
    acc._done = 0
    for segment, s in (("permutation_set", 0), ("lookup_set", 0), ("divide", 0), ("head", 1)):
        try:
            acc._turn(segment, s)
        except pkg.AeswError as e:
            assert e.status == api.ERR_INVALID_ARG and "head(0) comes next" in str(e)
        else:
            raise AssertionError((segment, s))
    assert acc._turn("head") == 0
    acc._done = 5
    try:
        acc._turn("divide")
    except pkg.AeswError as e:
        assert "complete" in str(e)
    else:
        raise AssertionError("divide twice")
    assert api.permutation_sets(4, 3) == 5 and [api.permutation_source(2, c) for c in range(8)] == \
        [("advice", 0), ("advice", 1), ("advice", 2), ("advice", 6), ("rcon", 0), ("advice", 3), ("advice", 4), ("advice", 5)]


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.VANISH_LIB_PATH, vc.launched())
    assert len(vc.launched()) == 14
    for name, words in (("test_gpu_vanish_cells.py", ("vc.FULL", "vc.SPLIT", "vc.STORE_MODES", "vanishing_tables", "vanishing_scalars", "quotient_accumulator", "quotient_extended")),
                        ("test_gpu_vanish_calls.py", ("aesw_vanish_%s_device", "head", "perm", "lookup", "divide", "torch.cuda.graph"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == vc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output cell is stored, never added to
        assert row["mad_u64"] >= 2 * 64, (name, row)    # every kernel multiplies in the field: a product is 2 x 8 x 8 limb products
        if "scalars" not in name:
            assert row["global_stores"] == 2, (name, row)  # one cell per lane, two 16-byte pieces
    cl.assert_tracked(table, TABLE)
