"""libaesw_sigma.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_sigma_ functions include/aesw_sigma.h declares, api.SIGMA_SYMBOLS binds
    exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * a Group refuses;
  * every __global__ in it is launched by the GPU tests (tests/sigma_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds; compared
    with the tracked table profiles/isa_resources_sigma.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_sigma_library.py).  The chunk and the scan kernel hold more than 256
    unified registers -- one wave per SIMD ("Not done") -- so the table's bound is 512 here;
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import sigma_cases as sc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_sigma.json"
code_object = cl.code_object_fixture("SIGMA_LIB_PATH")
DECLARED = ["aesw_sigma_columns", "aesw_sigma_mapping_host", "aesw_sigma_product_device", "aesw_sigma_sources_host", "aesw_sigma_tables_bytes",
            "aesw_sigma_tables_device", "aesw_sigma_workspace_bytes"]
METHODS = ("permutation_tables", "permutation_product")


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "sigma", DECLARED)
    for name in ("permutation_columns", "permutation_sources", "permutation_mapping", "load_sigma_library", "sigma_report_dict"):
        assert callable(getattr(pkg.api, name)), name
    header = (cl.ROOT / "include" / "aesw_sigma.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "sigma", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "sigma", ("sigma_scan_kernel", "sigma_chunk_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


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
