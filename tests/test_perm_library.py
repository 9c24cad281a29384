"""libaesw_perm.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_perm_ functions include/aesw_perm.h declares, api.PERM_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN (and no other library of the project is one),
    and the Python face is there;
  * every __global__ in it is launched by the GPU tests (tests/perm_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic at all, the scan's LDS two small arrays; compared with the tracked table
    profiles/isa_resources_perm.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest
    tests/test_perm_library.py);
  * aesw_perm_workspace_bytes is the rule header's layout;
  * the other libraries and their headers carry none of the new symbols."""
import check_library as cl
import perm_cases as pc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_perm.json"
code_object = cl.code_object_fixture("PERM_LIB_PATH")
DECLARED = ["aesw_perm_build_device", "aesw_perm_gather_fr_device", "aesw_perm_workspace_bytes"]
METHODS = ("permuted_columns", "gather_fr")


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "perm", DECLARED)
    assert callable(pkg.api.MultiplicityAccumulator.permuted_columns)
    header = (cl.ROOT / "include" / "aesw_perm.h").read_text()
    assert '#include "aesw_mult.h"' in header and "aesw_acc.h\"" not in header


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "perm", tmp_path)


def test_the_workspace_is_the_rule_headers(pkg):
    size = pkg.api.load_perm_library().aesw_perm_workspace_bytes
    per_set = 4 * (3 * (65536 + 4 * 256) + 32)  # three arrays per argument, as long as its section; 32 words of scalars
    assert [size(n) for n in (0, 1, 2, 1024, 1025)] == [0, per_set, 2 * per_set, 1024 * per_set, 0] and per_set % 16 == 0


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "perm", ("perm_scan_kernel", "perm_expand_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.PERM_LIB_PATH, pc.launched())
    assert len(pc.launched()) == 5
    src = (cl.ROOT / "tests" / "test_gpu_perm.py").read_text()
    assert all(name in src for name in ("pc.US", "pc.PAD_ROWS", "pc.GATHER_CELLS", "pc.STORE_MODES"))


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier")
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == pc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0 and row["sgpr_spill"] == 0, (name, row)  # every output word is stored, never added to
    scan, expand = table["aesw_perm::perm_scan_kernel"], table["aesw_perm::perm_expand_kernel"]
    assert scan["static_lds"] == 2 * 16 * 4 and scan["barriers"] >= 2 and scan["vgpr"] <= 64, scan  # 1 024 threads: 8 waves per SIMD at 64
    assert expand["global_stores"] >= 2 and expand["static_lds"] <= 64, expand
    for mode in pc.STORE_MODES:
        row = table["aesw_perm::perm_gather_fr_kernel<%d>" % mode]
        assert row["global_stores"] == 1 and row["global_loads"] == 2 and row["static_lds"] == 0 and row["lds_ops"] == 0, (mode, row)
    cl.assert_tracked(table, TABLE)
