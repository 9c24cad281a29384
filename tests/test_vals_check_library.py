"""libaesw_vals.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_vals.h declares, its NEEDED entry is
    libaesw.so via $ORIGIN, and the Python face (Context.check_values) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/vals_check_cases.py), and that list names
    nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, compared with the tracked table
    profiles/isa_resources_vals.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_vals_check_library.py;
  * the other libraries carry none of the new symbols; the one header that names the library is aesw_vacc.h, built over its rules.

The checks every checker library gets are in tests/check_library.py."""
import check_library as cl
import vals_check_cases as vcs
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_vals.json"
code_object = cl.code_object_fixture("VALS_LIB_PATH")
METHODS = ("check_values",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    declared = cl.check_exports(pkg, "vals")
    assert {"aesw_vals_check_device", "aesw_vals_check_rows", "aesw_vals_check_table", "aesw_vals_image_bytes"} <= set(declared), declared


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "vals", ("vals_check_kernel",), named_by=("aesw_vacc.h",))
    assert not [h.name for h in (cl.ROOT / "include").glob("*.h") if "vals_check_kernel" in h.read_text()]


def test_a_group_refuses_the_values_check(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.VALS_LIB_PATH, vcs.launched())
    assert vcs.launched() == {"aesw_vals::vals_check_kernel<false>", "aesw_vals::vals_check_kernel<true>", "aesw_vals::vals_report_init_kernel"}
    src = (cl.ROOT / "tests" / "test_gpu_vals_check.py").read_text()
    assert "vcs.KEY_MODES" in src and "vcs.SIZES" in src and "vcs.TABLE_SETS" in src


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    for kernel, ins in cl.instructions(code_object).items():
        if "vals_check_kernel" in kernel:  # a block travels as 16-byte loads
            assert sum(1 for t in ins if t.startswith("global_load_dwordx4")) >= 4, "%s: no 16-byte loads" % kernel
    table = cl.resource_table(code_object, cl.GLOBAL_COLUMNS)
    assert set(table) == vcs.launched(), sorted(table)
    cl.assert_tracked(table, TABLE)
