"""libaesw_quot.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_quot_ functions include/aesw_quot.h declares, api.QUOT_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one; it is the one entry of
    _build.QUOTIENT_LIBRARIES, a fifth table that library_names() and domain_library_names() do not list and library_entry() knows;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/quot_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds, at most 256
    unified registers, no LDS; compared with the tracked table profiles/isa_resources_quot.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_quot_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import importlib.util
import subprocess

import pytest

import check_library as cl
import quot_cases as qc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_quot.json"
code_object = cl.code_object_fixture("QUOT_LIB_PATH")
DECLARED = ["aesw_quot_sigma_fr_device"]
OTHERS = ("LIB_PATH", "CIRC_LIB_PATH", "COLS_LIB_PATH", "VALS_LIB_PATH", "ACC_LIB_PATH", "VACC_LIB_PATH", "MULT_LIB_PATH", "PERM_LIB_PATH", "THETA_LIB_PATH",
          "GRAND_LIB_PATH", "SIGMA_LIB_PATH", "NTT_LIB_PATH", "HOST_LIB_PATH")
METHODS = ("permutation_columns_fr",)


def _build_module():
    spec = importlib.util.spec_from_file_location("b", cl.ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.QUOT_LIB_PATH
    assert lib.name == "libaesw_quot.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = cl.declared("aesw_quot.h", "aesw_quot_")
    assert decl == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    loaded = api.load_quot_library()
    assert api.load_quot_library() is loaded
    assert sorted(api.QUOT_SYMBOLS) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES["quot"][:2] == (lib, api.QUOT_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    others = ("libaesw_acc", "libaesw_vacc", "libaesw_mult", "libaesw_perm", "libaesw_theta", "libaesw_grand", "libaesw_sigma", "libaesw_ntt", "libaesw_vals",
              "libaesw_circ", "libaesw_cols", "libaesw_host")
    assert not [s for s in others if s in dyn], dyn
    assert (cl.ROOT / "halo2-aes_amd" / "csrc" / "quot" / "aesw_quot.hip").exists()  # one level below csrc/, as every satellite's
    for name in METHODS:
        assert callable(getattr(api.Context, name)), name
    header = (cl.ROOT / "include" / "aesw_quot.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "NOT PINNED" in header and "NOT part of this library" in header  # what is unpinned, and that the evaluation has no kernel yet


def test_the_entry_is_a_fifth_table_and_the_four_stay_what_they_are():
    b = _build_module()
    assert list(b.QUOTIENT_LIBRARIES) == ["quot"] == b.quotient_library_names() and b.QUOT_LIB == b.PKG / "libaesw_quot.so"
    assert b.library_names() == list(b.SATELLITES) + list(b.FIELD_LIBRARIES) + list(b.ARGUMENT_LIBRARIES) and "quot" not in b.library_names()
    assert b.domain_library_names() == ["ntt"] == list(b.DOMAIN_LIBRARIES)
    assert list(b.SATELLITES) == ["circ", "cols", "vals", "acc", "perm", "vacc", "mult"] and list(b.FIELD_LIBRARIES) == ["theta"]
    assert list(b.ARGUMENT_LIBRARIES) == ["grand", "sigma"]
    sources, headers, public = b.library_entry("quot")
    assert sources[0].parent.name == "quot" and public.name == "aesw_quot.h" and headers[-1].name == "aesw_quot.h" and headers[0].name == "aesw_fr.h"
    assert all(h.exists() for h in headers)
    assert b.library_entry("ntt")[2].name == "aesw_ntt.h"
    with pytest.raises(KeyError):
        b.library_entry("nowhere")


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    missing = tmp_path / "nowhere" / pkg.api.QUOT_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        pkg.api.load_quot_library(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def test_the_other_libraries_are_left_alone(pkg):
    for other in OTHERS:
        text = cl.nm(getattr(pkg.api, other), "-C")
        assert "aesw_quot" not in text and "quot_sigma_kernel" not in text, other
    for header in sorted((cl.ROOT / "include").glob("*.h")):
        if header.name != "aesw_quot.h":
            assert "aesw_quot" not in header.read_text(), header.name


def test_a_group_refuses(pkg):
    for name in METHODS:
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, name)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.QUOT_LIB_PATH, qc.launched())
    assert len(qc.launched()) == 1
    for name, words in (("test_gpu_quot_sigma.py", ("qc.SIGMA_FR",)),):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == qc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output cell is stored, never added to
        assert row["mad_u64"] >= 2 * 64, (name, row)    # every kernel multiplies in the field: a product is 2 x 8 x 8 limb products
        assert row["static_lds"] == 0 and row["lds_ops"] == 0 and row["barriers"] == 0, (name, row)
        assert row["global_stores"] == 2, (name, row)   # one cell per thread, two 16-byte pieces
    cl.assert_tracked(table, TABLE)
