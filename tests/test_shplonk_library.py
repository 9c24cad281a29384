"""libaesw_shplonk.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_shplonk_ functions include/aesw_shplonk.h declares, api.SHPLONK_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * it is the entry of the fourth build table, _build.MULTIOPEN_LIBRARIES, and of api._MULTIOPEN_LIBRARIES -- not of the first three,
    which stay what their tests pin -- and build() builds it through build_multiopen, last, and loads it;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/shplonk_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic, the field products as 64-bit multiply-adds, at most 256 unified
    registers, LDS and barriers only in the kernels whose waves or threads meet, one 128-byte store a lane in the scan kernel;
    compared with the tracked table profiles/isa_resources_shplonk.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_shplonk_library.py);
  * the other libraries carry none of the new symbols, and the header names no other library."""
import subprocess

import check_library as cl
import shplonk_cases as sc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_shplonk.json"
code_object = cl.code_object_fixture("SHPLONK_LIB_PATH")
DECLARED = ["aesw_shplonk_combine_device", "aesw_shplonk_finish_device", "aesw_shplonk_prepare_device", "aesw_shplonk_quotient_device", "aesw_shplonk_report_bytes",
            "aesw_shplonk_scalars_bytes", "aesw_shplonk_scalars_offset", "aesw_shplonk_workspace_bytes"]
METHODS = ("shplonk_table", "shplonk_prepare", "shplonk_finish", "combine_columns", "set_quotient", "open_shplonk")
MEETING = ("prepare", "finish", "chunk", "carry", "scan")  # the kernels whose waves, or threads, meet through LDS


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.SHPLONK_LIB_PATH
    assert lib.name == "libaesw_shplonk.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    assert cl.declared("aesw_shplonk.h", "aesw_shplonk_") == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == DECLARED, sorted(exported)[:20]
    loaded = api.load_shplonk_library()
    assert api.load_shplonk_library() is loaded and sorted(api.SHPLONK_SYMBOLS) == DECLARED and all(getattr(loaded, f) is not None for f in DECLARED)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = cl.build_module()
    assert not [n for n in b.library_names() + b.curve_library_names() + b.proof_library_names() + ["host"] if "libaesw_%s" % n in dyn], dyn
    source = (cl.ROOT / "halo2-aes_amd" / "csrc" / "shplonk" / "aesw_shplonk.hip").read_text()
    assert "namespace aesw_shplonk {" in source and all('#include "../%s"' % h in source for h in ("aesw_fr_dev.h", "aesw_open.h", "aesw_shplonk.h"))
    header = (cl.ROOT / "include" / "aesw_shplonk.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1 and "NOT PINNED" in header and "halo2 orders the point sets by the value" in header
    assert not [n for n in b.library_names() + b.curve_library_names() + b.proof_library_names() if "aesw_" + n in header]


def test_the_fourth_table_has_the_shape_of_the_first_and_build_walks_it_last(pkg, monkeypatch):
    import __graft_entry__ as ge
    b, api = cl.build_module(), pkg.api
    assert b.multiopen_library_names() == ["shplonk"] == list(b.MULTIOPEN_LIBRARIES) == list(api._MULTIOPEN_LIBRARIES)
    assert not [t for t in (b.LIBRARIES, b.CURVE_LIBRARIES, b.PROOF_LIBRARIES, api._LIBRARIES, api._CURVE_LIBRARIES, api._PROOF_LIBRARIES) if "shplonk" in t]
    # the first three tables stay what their tests pin
    assert len(b.LIBRARIES) == 13 and len(api._LIBRARIES) == 15 and list(b.CURVE_LIBRARIES) == ["msm"] == list(api._CURVE_LIBRARIES)
    assert list(b.PROOF_LIBRARIES) == ["transcript"] == list(api._PROOF_LIBRARIES)
    sources, headers, public = b.MULTIOPEN_LIBRARIES["shplonk"]
    assert sources and all(s.exists() and s.parent == b.CSRC / "shplonk" and s.suffix == ".hip" for s in sources)
    assert [h.name for h in headers] == ["aesw_fr.h", "aesw_open.h", "aesw_shplonk.h"] and all(h.exists() and h.parent == b.CSRC for h in headers)
    assert public == b.INCLUDE / "aesw_shplonk.h" and public.exists()
    assert api._MULTIOPEN_LIBRARIES["shplonk"] == (api.SHPLONK_LIB_PATH, api.SHPLONK_SYMBOLS, api._NO_FALLBACK)
    built, loaded = [], []
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    monkeypatch.setattr(b, "build_curve", lambda name, force=False: built.append("curve:" + name))
    monkeypatch.setattr(b, "build_proof", lambda name, force=False: built.append("proof:" + name))
    monkeypatch.setattr(b, "build_multiopen", lambda name, force=False: built.append("multiopen:" + name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    for name in ("transcript", "shplonk"):
        monkeypatch.setattr(api, "load_%s_library" % name, lambda path=None, name=name: loaded.append(name))
    ge.build()
    assert built == b.library_names() + ["curve:msm", "proof:transcript", "multiopen:shplonk"] and loaded == ["transcript", "shplonk"]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "shplonk", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    others = dict(pkg.api._LIBRARIES, **pkg.api._CURVE_LIBRARIES, **pkg.api._PROOF_LIBRARIES)
    for other, (path, _symbols, _hint) in others.items():
        text = cl.nm(path, "-C")
        assert not [w for w in ("aesw_shplonk", "shplonk_prepare_kernel", "shplonk_scan_kernel", "shplonk_combine_kernel") if w in text], other
    naming = sorted(h.name for h in (cl.ROOT / "include").glob("*.h") if h.name != "aesw_shplonk.h" and "aesw_shplonk" in h.read_text())
    assert naming == []


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.SHPLONK_LIB_PATH, sc.launched())
    assert len(sc.launched()) == 12
    for name, words in (("test_gpu_shplonk_columns.py", ("sc.KS", "sc.STORE_MODES", "sc.stage", "shplonk_prepare", "shplonk_finish", "combine_columns", "set_quotient")),
                        ("test_gpu_shplonk_extents.py", ("sc.full_stage", "sc.u_on_a_point", "sc.degenerate_stages", "sc.WIDE_COLS", "run_stage", "check_stage")),
                        ("test_gpu_shplonk_reach.py", ("sc.REACH_K",)), ("test_gpu_shplonk_chain.py", ("sc.CHAIN_ROTATIONS", "open_shplonk"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == sc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
        if "report" not in name:
            assert row["mad_u64"] >= 2 * 64, (name, row)  # every other kernel multiplies in the field: a product is 2 x 8 x 8 limb products
        if any("shplonk_%s_kernel" % k in name for k in MEETING):
            assert row["static_lds"] > 0, (name, row)
        else:  # a thread of the powers, the combine and the report kernel meets no other
            assert row["static_lds"] == 0 and row["barriers"] == 0, (name, row)
        if "scan" in name:
            assert row["global_stores"] == 8, (name, row)  # a lane's four cells, two 16-byte pieces each: one 128-byte store a lane
        if "combine" in name:
            assert row["global_stores"] == 2, (name, row)
    cl.assert_tracked(table, TABLE)
