"""libaesw_acc.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_acc_ functions include/aesw_acc.h declares, api.ACC_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN (and no other library of the project is one), and the Python face is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/acc_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, at most 160 KiB of static LDS; compared with the
    tracked table profiles/isa_resources_acc.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest
    tests/test_acc_library.py);
  * aesw_acc_default_chunk is a function of the shape alone and never 0;
  * the other libraries carry none of the new symbols; the headers that name the library are the two built over it."""
import acc_cases as ac
import check_library as cl
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_acc.json"
code_object = cl.code_object_fixture("ACC_LIB_PATH")
DECLARED = ["aesw_acc_add_device", "aesw_acc_add_device_chunk", "aesw_acc_add_key_device", "aesw_acc_default_chunk", "aesw_acc_reset_device"]
METHODS = ("multiplicity_accumulator",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "acc", DECLARED)
    for method in ("reset", "add", "add_key", "histograms", "report"):
        assert callable(getattr(pkg.api.MultiplicityAccumulator, method)), method


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "acc", tmp_path)


def test_the_default_chunk_depends_on_the_shape_alone_and_is_never_zero(pkg):
    chunk = pkg.api.load_acc_library().aesw_acc_default_chunk
    # a chunk is at least 256 blocks (its Xor lookups dwarf the 65 536-word flush) ...
    assert chunk(14, 3, 0, 34) == 256 and chunk(14, 3, 7, 1) == 256 and chunk(20, 4, 0, 3083) == 256
    # ... and above that a run is spread over 128 pairs of workgroups: one circuit at K = 24 / N = 4, and a 2^15-block stream chunk
    cap = pkg.block_capacity(24, 4)
    assert cap == 49342 and chunk(24, 4, 0, cap) == 386 and chunk(24, 4, 0, 1 << 15) == 256 and chunk(24, 4, 1 << 15, cap - (1 << 15)) == 256
    assert chunk(30, 1024, 0, pkg.block_capacity(30, 1024)) == -(-pkg.block_capacity(30, 1024) // 128)
    assert chunk(12, 1, 0, 0) >= 1
    for k, n_sets, first, n in ((9, 1, 0, 0), (12, 2, 3, 1), (16, 3, 5, 100), (24, 4, 0, 40000), (30, 7, 1 << 20, 1 << 22)):
        got = chunk(k, n_sets, first, n)
        assert got >= 1 and got == chunk(k, n_sets, first, n), (k, n_sets, first, n)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "acc", ("acc_add_kernel",), named_by=("aesw_perm.h", "aesw_vacc.h"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.ACC_LIB_PATH, ac.launched())
    assert len(ac.launched()) == 5
    src = (cl.ROOT / "tests" / "test_gpu_acc.py").read_text()
    assert all(name in src for name in ("ac.SHAPES", "ac.LAYOUTS", "ac.TABLE_SETS", "ac.FORCED_CHUNKS", "ac.CONTENTION", "ac.ragged"))


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_adds="ds_add_u32")
    table = cl.resource_table(code_object, columns)
    assert set(table) == ac.launched(), sorted(table)
    for kernel, row in table.items():
        assert row["static_lds"] <= 160 * 1024, (kernel, row)
        if "acc_add_kernel" in kernel:
            # the counters: LDS adds, one per row step; global atomics: the flushes of the Xor half and of the two small ranges, and
            # the three words of the report
            assert row["lds_adds"] >= 22 and 3 + 3 <= row["global_atomics"] and 132 * 1024 < row["static_lds"], (kernel, row)
        elif "acc_reset_kernel" in kernel:
            assert row["global_atomics"] == 0 and row["lds_adds"] == 0 and row["global_stores"] >= 2, (kernel, row)
        else:
            assert row["lds_adds"] == 0 and row["global_atomics"] >= 1 + 3, (kernel, row)
    cl.assert_tracked(table, TABLE)
