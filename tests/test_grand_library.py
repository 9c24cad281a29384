"""libaesw_grand.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_grand_ functions include/aesw_grand.h declares, api.GRAND_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one; it is the first entry
    of _build.ARGUMENT_LIBRARIES, and _build.SATELLITES and _build.FIELD_LIBRARIES are what they were;
  * a Group refuses; the workspace function's zeros and its multiple of 16;
  * every __global__ in it is launched by the GPU tests (tests/grand_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, no atomic in any kernel, the field products as
    64-bit multiply-adds; compared with the tracked table profiles/isa_resources_grand.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_grand_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import importlib.util
import subprocess

import pytest

import check_library as cl
import grand_cases as gc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_grand.json"
code_object = cl.code_object_fixture("GRAND_LIB_PATH")
DECLARED = ["aesw_grand_invert_table_device", "aesw_grand_product_device", "aesw_grand_workspace_bytes"]
OTHERS = ("LIB_PATH", "CIRC_LIB_PATH", "COLS_LIB_PATH", "VALS_LIB_PATH", "ACC_LIB_PATH", "VACC_LIB_PATH", "MULT_LIB_PATH", "PERM_LIB_PATH", "THETA_LIB_PATH",
          "HOST_LIB_PATH")
OTHER_LIBRARIES_IN_WORDS = ("aesw_theta", "aesw_perm", "aesw_vacc", "aesw_acc", "aesw_circ", "aesw_cols", "aesw_vals")


def _build_module():
    spec = importlib.util.spec_from_file_location("b", cl.ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.GRAND_LIB_PATH
    assert lib.name == "libaesw_grand.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = cl.declared("aesw_grand.h", "aesw_grand_")
    assert decl == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    loaded = api.load_grand_library()
    assert api.load_grand_library() is loaded
    assert sorted(api.GRAND_SYMBOLS) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES["grand"][:2] == (lib, api.GRAND_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    others = ("libaesw_acc", "libaesw_vacc", "libaesw_mult", "libaesw_perm", "libaesw_theta", "libaesw_vals", "libaesw_circ", "libaesw_cols", "libaesw_host")
    assert not [s for s in others if s in dyn], dyn
    assert (cl.ROOT / "halo2-aes_amd" / "csrc" / "grand" / "aesw_grand.hip").exists()  # one level below csrc/, as every satellite's
    for name in ("invert_table", "grand_product"):
        assert callable(getattr(api.Context, name)), name
    assert callable(api.grand_report_dict)
    header = (cl.ROOT / "include" / "aesw_grand.h").read_text()
    assert '#include "aesw_mult.h"' in header and header.count("#include \"aesw_") == 1
    assert not [w for w in OTHER_LIBRARIES_IN_WORDS if w in header]


def test_the_entry_sits_in_the_third_table_and_the_other_two_are_unchanged():
    b = _build_module()
    assert list(b.ARGUMENT_LIBRARIES)[0] == "grand" and b.GRAND_LIB == b.PKG / "libaesw_grand.so"
    assert list(b.SATELLITES) == ["circ", "cols", "vals", "acc", "perm", "vacc", "mult"] and list(b.FIELD_LIBRARIES) == ["theta"]
    assert b.library_names() == list(b.SATELLITES) + ["theta"] + list(b.ARGUMENT_LIBRARIES)
    for name in b.library_names():  # one lookup finds a name in any of the three tables
        sources, headers, public = b.library_entry(name)
        assert sources[0].parent.name == name and public.name == "aesw_%s.h" % name, name
    with pytest.raises(KeyError):
        b.library_entry("nowhere")
    sources, headers, public = b.ARGUMENT_LIBRARIES["grand"]
    assert [h.name for h in headers[:2]] == ["aesw_fr.h", "aesw_grand.h"]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    missing = tmp_path / "nowhere" / pkg.api.GRAND_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        pkg.api.load_grand_library(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def test_the_other_libraries_are_left_alone(pkg):
    for other in OTHERS:
        text = cl.nm(getattr(pkg.api, other), "-C")
        assert "aesw_grand" not in text and "grand_scan_kernel" not in text and "grand_invert_kernel" not in text, other
    for header in sorted((cl.ROOT / "include").glob("*.h")):
        if header.name != "aesw_grand.h":
            assert "aesw_grand" not in header.read_text(), header.name


def test_a_group_refuses(pkg):
    for name in ("invert_table", "grand_product"):
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, name)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


def test_the_workspace_is_zero_outside_the_ranges_and_a_multiple_of_16(pkg):
    ws = pkg.api.load_grand_library().aesw_grand_workspace_bytes
    for k, n_sets in ((16, 1), (31, 1), (0, 1), (17, 0), (17, 1025), (2 ** 32 - 1, 1)):
        assert ws(k, n_sets) == 0, (k, n_sets)
    for k in (17, 18, 20, 30):
        for n_sets in (1, 2, 3, 1024):
            b = int(ws(k, n_sets))
            assert b > 0 and b % 16 == 0 and b >= 5 * n_sets * 48, (k, n_sets)
    assert ws(18, 1) > ws(17, 1) and ws(17, 2) == 2 * ws(17, 1)


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.GRAND_LIB_PATH, gc.launched())
    assert len(gc.launched()) == 8
    for name, words in (("test_gpu_grand_invert.py", ("gc.CHALLENGE_SEEDS", "gc.NONCANONICAL", "gc.ZERO_TERM_ROW")),
                        ("test_gpu_grand_product.py", ("gc.PRODUCT_ROWS", "gc.PAD_ROWS", "gc.STORE_MODES"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == gc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
    for name in ("grand_invert_kernel", "grand_chunk_kernel", "grand_carry_kernel") + tuple("grand_scan_kernel<%d>" % m for m in gc.STORE_MODES):
        assert table["aesw_grand::" + name]["mad_u64"] >= 2 * 64, (name, table["aesw_grand::" + name])  # a product is 2 x 8 x 8 limb products
    for mode in gc.STORE_MODES:
        row = table["aesw_grand::grand_scan_kernel<%d>" % mode]
        assert row["static_lds"] == 4 * 32 and row["barriers"] == 1, (mode, row)  # one cell per wave, one join
    cl.assert_tracked(table, TABLE)
