"""libaesw_msm.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_msm_ functions include/aesw_msm.h declares, api.MSM_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * it is an entry of the second build table, _build.CURVE_LIBRARIES, and of api._CURVE_LIBRARIES -- not of the first ones, which
    stay the thirteen and the fifteen -- and build() builds it through build_curve and loads it;
  * a Group refuses; a missing path says how to build it; fq_cell, g1_generator and g1_from_cells are the model's;
  * every __global__ in it is launched by the GPU tests (tests/msm_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no global atomic outside the basis call's report, the field products as 64-bit
    multiply-adds, the LDS atomics of the counting sort in the bucket kernel alone; the register counts are what they come to, at most
    the 512 a workgroup of 256 threads can hold a thread; compared with the tracked table profiles/isa_resources_msm.json
    (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_msm_library.py);
  * the other libraries carry none of the new symbols, and the header names no other library."""
import subprocess

import numpy as np

import check_library as cl
import msm_cases as mc
import msm_model as mm
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_msm.json"
code_object = cl.code_object_fixture("MSM_LIB_PATH")
DECLARED = ["aesw_msm_basis_device", "aesw_msm_chunk_rows", "aesw_msm_commit_device", "aesw_msm_slices", "aesw_msm_workspace_bytes"]
METHODS = ("msm_basis", "commit_columns")
MAX_UNIFIED = 512  # the registers of a SIMD over the one wave of a 256-thread workgroup it runs: the stated bound


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.MSM_LIB_PATH
    assert lib.name == "libaesw_msm.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    assert cl.declared("aesw_msm.h", "aesw_msm_") == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == DECLARED, sorted(exported)[:20]
    loaded = api.load_msm_library()
    assert api.load_msm_library() is loaded and sorted(api.MSM_SYMBOLS) == DECLARED and all(getattr(loaded, f) is not None for f in DECLARED)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = cl.build_module()
    assert not [n for n in b.library_names() + ["host"] if "libaesw_%s" % n in dyn], dyn
    source = cl.ROOT / "halo2-aes_amd" / "csrc" / "msm" / "aesw_msm.hip"
    assert "namespace aesw_msm {" in source.read_text() and '#include "../aesw_msm.h"' in source.read_text()
    header = (cl.ROOT / "include" / "aesw_msm.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1 and "NON-CANONICAL" in header
    assert not [n for n in b.library_names() if "aesw_" + n in header]


def test_the_second_table_has_the_shape_of_the_first_and_build_walks_it(pkg, monkeypatch):
    import __graft_entry__ as ge
    b, api = cl.build_module(), pkg.api
    assert b.curve_library_names() == ["msm"] == list(b.CURVE_LIBRARIES) == list(api._CURVE_LIBRARIES)
    assert "msm" not in b.LIBRARIES and "msm" not in api._LIBRARIES and len(b.LIBRARIES) == 13 and len(api._LIBRARIES) == 15
    sources, headers, public = b.CURVE_LIBRARIES["msm"]
    assert sources and all(s.exists() and s.parent == b.CSRC / "msm" and s.suffix == ".hip" for s in sources)
    assert [h.name for h in headers] == ["aesw_fr.h", "aesw_fq.h", "aesw_msm.h"] and all(h.exists() and h.parent == b.CSRC for h in headers)
    assert public == b.INCLUDE / "aesw_msm.h" and public.exists()
    assert api._CURVE_LIBRARIES["msm"] == (api.MSM_LIB_PATH, api.MSM_SYMBOLS, api._NO_FALLBACK)
    assert sorted(p.name for p in b.CSRC.iterdir() if p.is_file() and p.suffix in (".hip", ".cpp")) == sorted(s.name for s in b.PRODUCT_SOURCES)
    assert not [name for name in vars(b) if name.endswith("_LIB") and name not in ("LIB", "HOST_LIB")]
    built, loaded = [], []
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    monkeypatch.setattr(b, "build_curve", lambda name, force=False: built.append("curve:" + name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    monkeypatch.setattr(api, "load_msm_library", lambda path=None: loaded.append("msm"))
    ge.build()
    assert built == b.library_names() + ["curve:msm"] and loaded == ["msm"]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "msm", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    for other, (path, _symbols, _hint) in pkg.api._LIBRARIES.items():
        text = cl.nm(path, "-C")
        assert not [w for w in ("aesw_msm",) + mc.KERNELS if w in text], other
    naming = sorted(h.name for h in (cl.ROOT / "include").glob("*.h") if h.name != "aesw_msm.h" and "aesw_msm" in h.read_text())
    assert naming == []


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_the_module_functions_are_the_models(pkg):
    api = pkg.api
    assert api.FQ_MODULUS == mm.Q and api.FR_MODULUS == mm.R
    for v in (0, 1, 2, mm.Q - 1, mm.Q + 5, -1):
        assert api.fq_cell(v).tobytes() == mm.fq_bytes(v % mm.Q) and api.fq_cell(v).dtype == np.uint8
    assert api.g1_generator().tobytes() == mm.to_points([mm.GENERATOR]).tobytes() and mm.on_curve(mm.GENERATOR)
    points = [None, mm.GENERATOR] + list(mm.known_basis(4))
    assert api.g1_from_cells(mm.to_points(points)) == points == mm.from_points(mm.to_points(points))
    assert api.g1_from_cells(api.g1_generator()) == [mm.GENERATOR]


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.MSM_LIB_PATH, mc.launched())
    for name, words in (("test_gpu_msm_columns.py", ("mc.KS", "mc.SLICES", "mc.COLS", "msm_basis")), ("test_gpu_msm_reach.py", ("aesw_msm_chunk_rows", "aesw_msm_slices"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), lds_atomics=lambda t: t.startswith("ds_add"), barriers="s_barrier",
                   mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns, max_unified=None)  # no scratch, no VGPR spills; the register bound is stated here
    assert set(table) == mc.launched(), sorted(table)
    for name, row in table.items():
        assert row["vgpr"] + row["agpr"] <= MAX_UNIFIED, (name, row)
        if "basis" not in name:  # the basis call's report is added to; every other word of memory is stored, once
            assert row["global_atomics"] == 0, (name, row)
        if "digits" in name:  # a product by the raw 1: the limb products with its seven zero limbs fold away, the reduction's 64 stay
            assert row["mad_u64"] >= 64, (name, row)
        elif "reset" not in name:
            assert row["mad_u64"] >= 2 * 64, (name, row)  # every other kernel multiplies in a field: a product is 2 x 8 x 8 limb products
        if "bucket" in name:
            assert row["lds_atomics"] >= 2 and row["barriers"] >= 4 and row["static_lds"] > 2 * 4096, (name, row)  # the histogram and the cursor; the rows of a chunk
        else:
            assert row["lds_atomics"] == 0, (name, row)
        if "combine" in name:
            assert row["global_stores"] == 4 and row["static_lds"] == 0, (name, row)  # one affine point
    cl.assert_tracked(table, TABLE)
