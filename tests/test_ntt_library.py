"""libaesw_ntt.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_ntt_ functions include/aesw_ntt.h declares, api.NTT_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/ntt_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds, at most 256
    unified registers; compared with the tracked table profiles/isa_resources_ntt.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_ntt_library.py);
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import ntt_cases as nc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_ntt.json"
code_object = cl.code_object_fixture("NTT_LIB_PATH")
DECLARED = ["aesw_ntt_coeff_to_extended_device", "aesw_ntt_coeff_to_lagrange_device", "aesw_ntt_extended_to_coeff_device", "aesw_ntt_lagrange_to_coeff_device",
            "aesw_ntt_tables_bytes", "aesw_ntt_tables_device", "aesw_ntt_workspace_bytes"]
METHODS = ("ntt_tables", "lagrange_to_coeff", "coeff_to_lagrange", "coeff_to_extended", "extended_to_coeff")


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "ntt", DECLARED)
    assert callable(pkg.api.load_ntt_library)
    header = (cl.ROOT / "include" / "aesw_ntt.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "NOT PINNED" in header and "NON-CANONICAL" in header


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "ntt", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "ntt", ("ntt_pass_kernel", "ntt_tables_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.NTT_LIB_PATH, nc.launched())
    assert len(nc.launched()) == 4
    for name, words in (("test_gpu_ntt_transform.py", ("nc.SHAPES", "nc.EXTENDED", "nc.STORE_MODES", "nc.TABLES_MAX_K")),
                        ("test_gpu_ntt_reach.py", ("nc.THREE_PASSES", "nc.BIG"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == nc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
        assert row["mad_u64"] >= 2 * 64, (name, row)    # every kernel multiplies in the field: a product is 2 x 8 x 8 limb products
        if "pass" in name:
            assert row["static_lds"] == 32 << nc.PASS_LOG and row["barriers"] >= 2, (name, row)  # one tile, limb-planar
    cl.assert_tracked(table, TABLE)
