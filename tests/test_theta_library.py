"""libaesw_theta.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_theta_ functions include/aesw_theta.h declares, api.THETA_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no satellite is one; it is the entry of
    _build.FIELD_LIBRARIES, and _build.SATELLITES still has its seven;
  * every __global__ in it is launched by the GPU tests (tests/theta_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, no atomic in any kernel -- the columns and the
    inputs kernel among them --, the products of the table kernel as 64-bit multiply-adds; compared with the tracked table
    profiles/isa_resources_theta.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest
    tests/test_theta_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import importlib.util
import subprocess

import pytest

import check_library as cl
import theta_cases as tc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_theta.json"
code_object = cl.code_object_fixture("THETA_LIB_PATH")
DECLARED = ["aesw_theta_columns_device", "aesw_theta_compress_table_device", "aesw_theta_inputs_device", "aesw_theta_prepare"]
OTHERS = ("LIB_PATH", "CIRC_LIB_PATH", "COLS_LIB_PATH", "VALS_LIB_PATH", "ACC_LIB_PATH", "VACC_LIB_PATH", "MULT_LIB_PATH", "PERM_LIB_PATH", "HOST_LIB_PATH")


def _build_module():
    spec = importlib.util.spec_from_file_location("b", cl.ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.THETA_LIB_PATH
    assert lib.name == "libaesw_theta.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = cl.declared("aesw_theta.h", "aesw_theta_")
    assert decl == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    loaded = api.load_theta_library()
    assert api.load_theta_library() is loaded
    assert sorted(api.THETA_SYMBOLS) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES["theta"][:2] == (lib, api.THETA_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    satellites = ("libaesw_acc", "libaesw_vacc", "libaesw_mult", "libaesw_perm", "libaesw_vals", "libaesw_circ", "libaesw_cols", "libaesw_host")
    assert not [s for s in satellites if s in dyn], dyn
    assert (cl.ROOT / "halo2-aes_amd" / "csrc" / "theta" / "aesw_theta.hip").exists()  # one level below csrc/, as every satellite's
    b = _build_module()
    assert len(b.SATELLITES) == 7 and "theta" not in b.SATELLITES
    assert list(b.FIELD_LIBRARIES) == ["theta"] and b.THETA_LIB == lib
    for name in ("compress_table", "lookup_inputs", "argument_columns"):
        assert callable(getattr(api.Context, name)), name
    header = (cl.ROOT / "include" / "aesw_theta.h").read_text()
    assert '#include "aesw_mult.h"' in header and "aesw_perm" not in header and "aesw_vacc" not in header


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    missing = tmp_path / "nowhere" / pkg.api.THETA_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        pkg.api.load_theta_library(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def test_the_other_libraries_are_left_alone(pkg):
    for other in OTHERS:
        text = cl.nm(getattr(pkg.api, other), "-C")
        assert "aesw_theta" not in text and "theta_table_kernel" not in text and "theta_inputs_kernel" not in text, other
    for header in sorted((cl.ROOT / "include").glob("*.h")):
        if header.name != "aesw_theta.h":
            assert "aesw_theta" not in header.read_text(), header.name


def test_a_group_refuses(pkg):
    for name in ("compress_table", "lookup_inputs", "argument_columns"):
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, name)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


def test_an_int_theta_becomes_its_montgomery_cell(pkg):
    api = pkg.api
    assert api.FR_MODULUS == tc.R
    for v in (0, 1, 2, tc.R - 1, tc.R, tc.R + 5, 1 << 255):
        cell = api.fr_cell(v)
        assert cell.shape == (32,) and int.from_bytes(cell.tobytes(), "little") == (v << 256) % tc.R


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.THETA_LIB_PATH, tc.launched())
    assert len(tc.launched()) == 6
    for name, words in (("test_gpu_theta_table.py", ("tc.THETA_SEEDS", "tc.NONCANONICAL")), ("test_gpu_theta_inputs.py", ("tc.INPUT_SHAPES",)),
                        ("test_gpu_theta_columns.py", ("tc.COLUMN_ROWS", "tc.PAD_ROWS", "tc.STORE_MODES"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == tc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
    compress, inputs = table["aesw_theta::theta_table_kernel"], table["aesw_theta::theta_inputs_kernel"]
    assert compress["mad_u64"] >= 3 * 2 * 64 and compress["static_lds"] == 0, compress  # three products of 2 x 8 x 8 limb products
    assert inputs["global_stores"] >= 6 and inputs["static_lds"] <= 64, inputs  # five pieces and the workgroup's part of the report
    for mode in tc.STORE_MODES:
        row = table["aesw_theta::theta_columns_kernel<%d>" % mode]
        assert row["global_stores"] == 1 and row["global_loads"] <= 2 and row["static_lds"] == 0 and row["lds_ops"] == 0, (mode, row)
    cl.assert_tracked(table, TABLE)
