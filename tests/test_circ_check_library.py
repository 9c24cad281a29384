"""libaesw_circ.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_circ.h declares, and the Python face
    (Context.check_circuits) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/circ_check_cases.py), and that list names
    nothing else: the separate library is no way round "no kernel ships unswept";
  * its code object: no scratch, no VGPR spills, at most 256 unified registers (twelve waves per CU, what check_kernel runs
    at), compared with the tracked table profiles/isa_resources_circ.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_circ_check_library.py;
  * libaesw.so is not touched: it holds no circ_check kernel and does not export the new entry point (its own kernel set and
    ISA table are pinned by the existing tests).

The checks every checker library gets are in tests/check_library.py."""
import check_library as cl
import circ_check_cases as ccc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_circ.json"
code_object = cl.code_object_fixture("CIRC_LIB_PATH")
METHODS = ("check_circuits",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    declared = cl.check_exports(pkg, "circ")
    assert "aesw_circ_check_witness_device" in declared and len(declared) >= 2, declared


def test_the_other_libraries_are_left_alone(pkg):
    # libaesw.so assembles many circuits in a namespace aesw_circ of its own: what no other library holds is the C prefix
    cl.check_others_left_alone(pkg, "circ", ("circ_check_kernel",), named_by=("aesw_cols.h", "aesw_vals.h"), symbol="aesw_circ_")


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_the_product_library_is_left_alone(pkg):
    text = cl.nm(pkg.api.LIB_PATH, "-C")
    assert "circ_check_kernel" not in text and "aesw_circ_check_witness_device" not in text
    assert not [ln for ln in (cl.ROOT / "include" / "aesw.h").read_text().splitlines() if "aesw_circ_check" in ln]


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.CIRC_LIB_PATH, ccc.launched())
    assert ccc.launched() == {"aesw_circ::circ_check_kernel<0>", "aesw_circ::circ_check_kernel<1>", "aesw_circ::circ_report_init_kernel"}
    # the GPU sweep really runs over that list
    src = (cl.ROOT / "tests" / "test_gpu_circ_check.py").read_text()
    assert "ccc.LAYOUTS" in src and "ccc.SHAPES" in src


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    for kernel, ins in cl.instructions(code_object).items():
        # the offsets are searched with scalar loads (the search runs once per block and wave)
        if "circ_check_kernel" in kernel:
            assert any(t.startswith("s_load_dwordx2") for t in ins[50:]), "%s: the circuit search has no scalar load" % kernel
    table = cl.resource_table(code_object, {"global_loads": "global_load_", "scalar_loads_x2": "s_load_dwordx2",
                                            "global_stores": "global_store_", "global_atomics": "global_atomic_"})
    assert set(table) == ccc.launched(), sorted(table)
    cl.assert_tracked(table, TABLE)
