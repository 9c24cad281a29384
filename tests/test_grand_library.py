"""libaesw_grand.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_grand_ functions include/aesw_grand.h declares, api.GRAND_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * a Group refuses; the workspace function's zeros and its multiple of 16;
  * every __global__ in it is launched by the GPU tests (tests/grand_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, no atomic in any kernel, the field products as
    64-bit multiply-adds; compared with the tracked table profiles/isa_resources_grand.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_grand_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import grand_cases as gc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_grand.json"
code_object = cl.code_object_fixture("GRAND_LIB_PATH")
DECLARED = ["aesw_grand_invert_table_device", "aesw_grand_product_device", "aesw_grand_workspace_bytes"]
OTHER_LIBRARIES_IN_WORDS = ("aesw_theta", "aesw_perm", "aesw_vacc", "aesw_acc", "aesw_circ", "aesw_cols", "aesw_vals")
METHODS = ("invert_table", "grand_product")


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "grand", DECLARED)
    assert callable(pkg.api.grand_report_dict)
    header = (cl.ROOT / "include" / "aesw_grand.h").read_text()
    assert '#include "aesw_mult.h"' in header and header.count("#include \"aesw_") == 1
    assert not [w for w in OTHER_LIBRARIES_IN_WORDS if w in header]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "grand", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "grand", ("grand_scan_kernel", "grand_invert_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


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
