"""libaesw_sigma.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_sigma_ functions include/aesw_sigma.h declares, api.SIGMA_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one; it is the second entry
    of _build.ARGUMENT_LIBRARIES, behind "grand";
  * a Group refuses;
  * every __global__ in it is launched by the GPU tests (tests/sigma_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds; compared
    with the tracked table profiles/isa_resources_sigma.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_sigma_library.py).  The chunk and the scan kernel hold more than 256
    unified registers -- one wave per SIMD ("Not done") -- so the table's bound is 512 here;
  * the other libraries and their headers carry none of the new symbols."""
import importlib.util
import subprocess

import pytest

import check_library as cl
import sigma_cases as sc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_sigma.json"
code_object = cl.code_object_fixture("SIGMA_LIB_PATH")
DECLARED = ["aesw_sigma_columns", "aesw_sigma_mapping_host", "aesw_sigma_product_device", "aesw_sigma_sources_host", "aesw_sigma_tables_bytes",
            "aesw_sigma_tables_device", "aesw_sigma_workspace_bytes"]
OTHERS = ("LIB_PATH", "CIRC_LIB_PATH", "COLS_LIB_PATH", "VALS_LIB_PATH", "ACC_LIB_PATH", "VACC_LIB_PATH", "MULT_LIB_PATH", "PERM_LIB_PATH", "THETA_LIB_PATH",
          "GRAND_LIB_PATH", "HOST_LIB_PATH")


def _build_module():
    spec = importlib.util.spec_from_file_location("b", cl.ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.SIGMA_LIB_PATH
    assert lib.name == "libaesw_sigma.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = cl.declared("aesw_sigma.h", "aesw_sigma_")
    assert decl == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    loaded = api.load_sigma_library()
    assert api.load_sigma_library() is loaded
    assert sorted(api.SIGMA_SYMBOLS) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES["sigma"][:2] == (lib, api.SIGMA_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    others = ("libaesw_acc", "libaesw_vacc", "libaesw_mult", "libaesw_perm", "libaesw_theta", "libaesw_grand", "libaesw_vals", "libaesw_circ", "libaesw_cols", "libaesw_host")
    assert not [s for s in others if s in dyn], dyn
    assert (cl.ROOT / "halo2-aes_amd" / "csrc" / "sigma" / "aesw_sigma.hip").exists()  # one level below csrc/, as every satellite's
    for name in ("permutation_tables", "permutation_product"):
        assert callable(getattr(api.Context, name)), name
    for name in ("permutation_columns", "permutation_sources", "permutation_mapping", "load_sigma_library", "sigma_report_dict"):
        assert callable(getattr(api, name)), name
    header = (cl.ROOT / "include" / "aesw_sigma.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1


def test_the_entry_is_the_second_of_the_argument_libraries():
    b = _build_module()
    assert list(b.ARGUMENT_LIBRARIES) == ["grand", "sigma"] and list(b.ARGUMENT_LIBRARIES)[1] == "sigma" and b.SIGMA_LIB == b.PKG / "libaesw_sigma.so"
    assert b.library_names()[-2:] == ["grand", "sigma"]
    sources, headers, public = b.library_entry("sigma")
    assert sources[0].parent.name == "sigma" and public.name == "aesw_sigma.h" and [h.name for h in headers] == ["aesw_fr.h", "aesw_sigma.h"]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    missing = tmp_path / "nowhere" / pkg.api.SIGMA_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        pkg.api.load_sigma_library(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def test_the_other_libraries_are_left_alone(pkg):
    for other in OTHERS:
        text = cl.nm(getattr(pkg.api, other), "-C")
        assert "aesw_sigma" not in text and "sigma_scan_kernel" not in text and "sigma_chunk_kernel" not in text, other
    for header in sorted((cl.ROOT / "include").glob("*.h")):
        if header.name != "aesw_sigma.h":
            assert "aesw_sigma" not in header.read_text(), header.name


def test_a_group_refuses(pkg):
    for name in ("permutation_tables", "permutation_product"):
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, name)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.SIGMA_LIB_PATH, sc.launched())
    assert len(sc.launched()) == 8
    for name, words in (("test_gpu_sigma_tables.py", ("sc.TABLE_KS", "sc.TABLE_COLS")),
                        ("test_gpu_sigma_product.py", ("sc.PRODUCTS", "sc.STORE_MODES", "sc.ZERO_CELL", "sc.NONCANONICAL"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns, max_unified=512)  # no scratch, no VGPR spills
    assert set(table) == sc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
        assert row["mad_u64"] >= 2 * 64, (name, row)    # every kernel multiplies in the field: a product is 2 x 8 x 8 limb products
    cl.assert_tracked(table, TABLE)
