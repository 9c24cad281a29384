"""libaesw_theta.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_theta_ functions include/aesw_theta.h declares, api.THETA_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * every __global__ in it is launched by the GPU tests (tests/theta_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, no atomic in any kernel -- the columns and the
    inputs kernel among them --, the products of the table kernel as 64-bit multiply-adds; compared with the tracked table
    profiles/isa_resources_theta.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest
    tests/test_theta_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import theta_cases as tc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_theta.json"
code_object = cl.code_object_fixture("THETA_LIB_PATH")
DECLARED = ["aesw_theta_columns_device", "aesw_theta_compress_table_device", "aesw_theta_inputs_device", "aesw_theta_prepare"]
METHODS = ("compress_table", "lookup_inputs", "argument_columns")


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "theta", DECLARED)
    header = (cl.ROOT / "include" / "aesw_theta.h").read_text()
    assert '#include "aesw_mult.h"' in header and "aesw_perm" not in header and "aesw_vacc" not in header


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "theta", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "theta", ("theta_table_kernel", "theta_inputs_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


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
