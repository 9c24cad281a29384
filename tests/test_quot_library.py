"""libaesw_quot.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_quot_ functions include/aesw_quot.h declares, api.QUOT_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/quot_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds, at most 256
    unified registers, no LDS; compared with the tracked table profiles/isa_resources_quot.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_quot_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import quot_cases as qc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_quot.json"
code_object = cl.code_object_fixture("QUOT_LIB_PATH")
DECLARED = ["aesw_quot_sigma_fr_device"]
METHODS = ("permutation_columns_fr",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "quot", DECLARED)
    header = (cl.ROOT / "include" / "aesw_quot.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "NOT PINNED" in header and "NOT part of this library" in header  # what is unpinned, and that the evaluation has no kernel yet


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "quot", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "quot", ("quot_sigma_kernel",))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


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
