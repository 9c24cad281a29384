"""libaesw_cols.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_cols.h declares, its NEEDED entry is
    libaesw.so via $ORIGIN, and the Python face (Context.check_columns) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/cols_check_cases.py), and that list names
    nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, compared with the tracked table
    profiles/isa_resources_cols.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_cols_check_library.py;
  * the other libraries and their headers carry none of the new symbols.

The checks every checker library gets are in tests/check_library.py."""
import check_library as cl
import cols_check_cases as ccs
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_cols.json"
code_object = cl.code_object_fixture("COLS_LIB_PATH")
METHODS = ("check_columns",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    declared = cl.check_exports(pkg, "cols")
    assert "aesw_cols_check_device" in declared and "aesw_cols_cell_index" in declared and len(declared) >= 5, declared


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "cols", ("cols_check_kernel",))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_the_cell_index_helper(pkg):
    lib = pkg.api.load_cols_library()
    assert lib.aesw_cols_cell_index(14, 1, 0, 0, 0) == 0
    assert lib.aesw_cols_cell_index(14, 1, 3, 2, 77) == ((3 * 4 + 2) << 14) + 77
    assert lib.aesw_cols_cell_index(30, 1024, 5, 3072, (1 << 30) - 1) == ((5 * 3073 + 3072) << 30) + (1 << 30) - 1


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.COLS_LIB_PATH, ccs.launched())
    assert ccs.launched() == {"aesw_cols::cols_check_kernel<false>", "aesw_cols::cols_check_kernel<true>", "aesw_cols::cols_report_init_kernel"}
    src = (cl.ROOT / "tests" / "test_gpu_cols_check.py").read_text()
    assert "ccs.FORMS" in src and "ccs.SHAPES" in src


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    for kernel, ins in cl.instructions(code_object).items():
        if "cols_check_kernel" in kernel:  # the circuit search and the sweep's offsets run on scalar loads
            assert any(t.startswith(("s_load_dwordx2", "s_load_dwordx4")) for t in ins[50:]), "%s: no scalar load of the offsets" % kernel
    table = cl.resource_table(code_object, cl.GLOBAL_COLUMNS)
    assert set(table) == ccs.launched(), sorted(table)
    cl.assert_tracked(table, TABLE)
