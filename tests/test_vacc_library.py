"""libaesw_vacc.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_vacc_ functions include/aesw_vacc.h declares, api.VACC_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN (and no other library of the project is one),
    and the Python face is there;
  * every __global__ in it is launched by the GPU sweep (tests/vacc_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, the counters and at most 160 KiB of static LDS, an
    LDS add per row step, the flushes and the report as global atomics; compared with the tracked table
    profiles/isa_resources_vacc.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest
    tests/test_vacc_library.py);
  * aesw_vacc_default_chunk is aesw_acc_default_chunk on the shapes of tests/test_acc_library.py;
  * the other libraries and their headers carry none of the new symbols, and the accumulator still refuses VALUES by name."""
import check_library as cl
import vacc_cases as vc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_vacc.json"
code_object = cl.code_object_fixture("VACC_LIB_PATH")
DECLARED = ["aesw_vacc_add_device", "aesw_vacc_add_device_chunk", "aesw_vacc_default_chunk", "aesw_vacc_prepare"]
METHODS = ("multiplicity_accumulator",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "vacc", DECLARED)
    assert callable(pkg.api.MultiplicityAccumulator.add_values)
    header = (cl.ROOT / "include" / "aesw_vacc.h").read_text()
    assert '#include "aesw_mult.h"' in header and "aesw_acc.h\"" not in header and "aesw_vals.h\"" not in header


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "vacc", tmp_path)


def test_an_accumulator_that_never_sees_values_does_not_load_the_library():
    """add_values loads libaesw_vacc.so on its first call: the constructor binds libaesw_acc.so alone."""
    import ast
    tree = ast.parse((cl.ROOT / "halo2-aes_amd" / "api.py").read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MultiplicityAccumulator")
    loads = {f.name: [c.func.id for c in ast.walk(f) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id.startswith("load_")]
             for f in cls.body if isinstance(f, ast.FunctionDef)}
    assert loads["add_values"] == ["load_vacc_library"] and loads["__init__"] == ["load_acc_library"]
    assert not [name for name, ls in loads.items() if "load_vacc_library" in ls and name != "add_values"]


def test_the_default_chunk_is_the_accumulators(pkg):
    chunk, acc_chunk = pkg.api.load_vacc_library().aesw_vacc_default_chunk, pkg.api.load_acc_library().aesw_acc_default_chunk
    cap = pkg.block_capacity(24, 4)
    big = pkg.block_capacity(30, 1024)
    shapes = ((14, 3, 0, 34), (14, 3, 7, 1), (20, 4, 0, 3083), (24, 4, 0, cap), (24, 4, 0, 1 << 15), (24, 4, 1 << 15, cap - (1 << 15)), (30, 1024, 0, big),
              (12, 1, 0, 0), (9, 1, 0, 0), (12, 2, 3, 1), (16, 3, 5, 100), (24, 4, 0, 40000), (30, 7, 1 << 20, 1 << 22))
    for shape in shapes:
        assert chunk(*shape) == acc_chunk(*shape) >= 1, shape
    assert chunk(14, 3, 0, 34) == 256 and chunk(24, 4, 0, cap) == 386 and chunk(30, 1024, 0, big) == -(-big // 128)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "vacc", ("vacc_count_kernel",))
    # every refusal of VALUES stays, by name
    acc = (cl.ROOT / "halo2-aes_amd" / "csrc" / "acc" / "aesw_acc.hip").read_text()
    rules = (cl.ROOT / "halo2-aes_amd" / "csrc" / "aesw_entry_rules.h").read_text()
    said = "the layout must be DENSE or PACKED (a VALUES witness has no x)"
    assert acc.count("bad_layout(layout)") == 2 and rules.count(said) == 1  # both entry points that take a layout; the text, once


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.VACC_LIB_PATH, vc.launched())
    assert len(vc.launched()) == 1
    src = (cl.ROOT / "tests" / "test_gpu_vacc.py").read_text()
    assert all(name in src for name in ("vc.SHAPES", "vc.TABLE_SETS", "vc.FORCED_CHUNKS", "vc.CONTENTION", "vc.ragged", "vc.CORRUPTIONS"))


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_adds="ds_add_u32")
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == vc.launched(), sorted(table)
    row = table["aesw_vacc::vacc_count_kernel"]
    # the counters: LDS adds, one per row step; global atomics: the flushes of the Xor half and of the two small ranges, and the
    # three words of the report; LDS: the counters and more, within a workgroup's 160 KiB
    assert row["lds_adds"] >= 17 and 3 + 3 <= row["global_atomics"] and 132 * 1024 < row["static_lds"] <= 160 * 1024, row
    assert row["global_stores"] == 0, row
    cl.assert_tracked(table, TABLE)
