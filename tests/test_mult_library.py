"""libaesw_mult.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_mult_ functions include/aesw_mult.h declares, api.MULT_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN, and the Python face (Context.lookup_multiplicities) is there;
  * the loader: the default path is cached, an explicit path is not, a missing path says how to build it;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/mult_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers; the PRIVATE form counts with LDS adds and has no
    global atomic but the report's, the DIRECT form is the one with global atomic adds; compared with the tracked table
    profiles/isa_resources_mult.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_mult_library.py);
  * the other libraries carry none of the new symbols; the headers that name the library are the five that include aesw_mult.h."""
import shutil

import pytest

import check_library as cl
import mult_cases as mc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_mult.json"
code_object = cl.code_object_fixture("MULT_LIB_PATH")
DECLARED = ["aesw_mult_bin", "aesw_mult_count_device", "aesw_mult_count_device_form", "aesw_mult_default_form"]
METHODS = ("lookup_multiplicities",)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "mult", DECLARED)
    assert ctypes_fields(pkg.api.MultReport) == ["lookups", "misses", "first_miss"]


def ctypes_fields(struct):
    return [n for n, _ in struct._fields_]


def test_the_loader_caches_the_default_and_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    api = pkg.api
    first = api.load_mult_library()
    assert api.load_mult_library() is first
    copy = shutil.copy(api.MULT_LIB_PATH, tmp_path / api.MULT_LIB_PATH.name)
    other = api.load_mult_library(copy)
    assert other is not first and api.load_mult_library(copy) is not other and api.load_mult_library() is first
    assert all(getattr(other, name).restype is res for name, (res, _args) in api.MULT_SYMBOLS.items())
    missing = tmp_path / "nowhere" / api.MULT_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        api.load_mult_library(missing)
    assert str(missing) in str(e.value) and "import __graft_entry__ as g; g.build()" in str(e.value)
    assert "There is no fallback implementation." in str(e.value)


def test_the_pure_host_functions(pkg):
    lib = pkg.api.load_mult_library()
    assert lib.aesw_mult_bin(1, 7, 9) == 7 and lib.aesw_mult_bin(3, 255, 0) == 256 + 255 and lib.aesw_mult_bin(2, 255, 255) == 66047
    assert lib.aesw_mult_bin(4, 0, 1) == 66048 and lib.aesw_mult_bin(5, 255, 1) == 66559 and lib.aesw_mult_bin(0, 0, 0) == 2 ** 32 - 1
    # the default form depends on the shape alone: PRIVATE from 128 workgroups (two per circuit and set) on
    assert lib.aesw_mult_default_form(23, 1, 1) == mc.FORM_DIRECT and lib.aesw_mult_default_form(20, 4, 340) == mc.FORM_PRIVATE
    assert lib.aesw_mult_default_form(12, 1, 63) == mc.FORM_DIRECT and lib.aesw_mult_default_form(12, 1, 64) == mc.FORM_PRIVATE
    assert [lib.aesw_mult_default_form(k, 2, 32) for k in (2, 12, 30)] == [mc.FORM_PRIVATE] * 3


def test_the_other_libraries_are_left_alone(pkg):
    # the multiplicity family and what compresses its table include aesw_mult.h (the row order, the bounds) and say so
    family = ("aesw_acc.h", "aesw_grand.h", "aesw_perm.h", "aesw_theta.h", "aesw_vacc.h")
    cl.check_others_left_alone(pkg, "mult", ("mult_private_kernel", "mult_direct_kernel"), named_by=family)


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.MULT_LIB_PATH, mc.launched())
    assert len(mc.launched()) == 5
    src = (cl.ROOT / "tests" / "test_gpu_mult.py").read_text()
    assert "mc.FORMS" in src and "mc.LAYOUTS" in src and "mc.TABLE_SETS" in src and "mc.SHAPES" in src and "mc.CONTENTION" in src


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_adds="ds_add_u32")
    table = cl.resource_table(code_object, columns)
    assert set(table) == mc.launched(), sorted(table)
    for kernel, row in table.items():
        if "mult_init_kernel" in kernel:
            assert row["global_atomics"] == 0 and row["lds_adds"] == 0 and row["global_stores"] >= 2
            continue
        ins = cl.instructions(code_object)[kernel]
        assert sum(1 for t in ins if t.startswith("global_load_dwordx4")) >= 3, "%s: a block travels as 16-byte loads" % kernel
        returning = [t for t in ins if t.startswith("global_atomic_") and " sc0" in t]  # nothing waits for an add's old value
        assert not returning, (kernel, returning[:3])
        if "private" in kernel:
            # the counters: LDS adds, one per row step and one for the key rows; global atomics: the three words of the report
            assert row["lds_adds"] >= 23 and row["global_atomics"] == 3, (kernel, row)
            assert 132 * 1024 < row["static_lds"] <= 160 * 1024, (kernel, row)
        else:
            assert row["lds_adds"] == 0 and row["global_atomics"] >= 23 + 3, (kernel, row)
    cl.assert_tracked(table, TABLE)
