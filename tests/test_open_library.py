"""libaesw_open.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_open_ functions include/aesw_open.h declares, api.OPEN_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * a Group refuses; a missing path says how to build it; rotated_points is x * omega_k^r in cells;
  * every __global__ in it is launched by the GPU tests (tests/open_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds, at most 256
    unified registers, LDS and barriers only in the kernels whose waves meet; compared with the tracked table
    profiles/isa_resources_open.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_open_library.py);
  * the other libraries and their headers carry none of the new symbols, and the header names no other library."""
import numpy as np
import pytest

import check_library as cl
import ntt_model as nm
import open_cases as oc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_open.json"
code_object = cl.code_object_fixture("OPEN_LIB_PATH")
DECLARED = ["aesw_open_divide_device", "aesw_open_evaluate_device", "aesw_open_fold_device", "aesw_open_workspace_bytes"]
OTHER_LIBRARIES_IN_WORDS = ("aesw_ntt", "aesw_quot", "aesw_grand", "aesw_sigma", "aesw_theta", "aesw_perm", "aesw_mult", "aesw_acc", "aesw_vacc", "aesw_vals",
                            "aesw_cols", "aesw_circ")
METHODS = ("evaluate_columns", "fold_columns", "divide_columns")
MEETING = ("open_chunk_kernel", "open_carry_kernel", "open_scan_kernel")  # the kernels whose waves meet through LDS


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    cl.check_exports(pkg, "open", DECLARED)
    source = cl.ROOT / "halo2-aes_amd" / "csrc" / "open" / "aesw_open.hip"
    assert "namespace aesw_open {" in source.read_text() and '#include "../aesw_fr_dev.h"' in source.read_text()
    header = (cl.ROOT / "include" / "aesw_open.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "NOT PINNED" in header and "NON-CANONICAL" in header
    assert not [w for w in OTHER_LIBRARIES_IN_WORDS if w in header]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "open", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    cl.check_others_left_alone(pkg, "open", ("open_chunk_kernel", "open_fold_kernel"))


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_rotated_points_are_the_cells_of_x_times_omega_to_the_rotation(pkg):
    k, x = 17, nm.seeded_values(1, 0x726f)[0]
    rotations = [0, 1, -1, 5, -(1 << k), (1 << k) + 3]
    cells = pkg.api.rotated_points(x, k, rotations)
    assert cells.dtype == np.uint8 and cells.shape == (len(rotations), 32)
    w = nm.omega(k)
    assert nm.from_cells(cells) == [x * pow(w, r, nm.R) % nm.R for r in rotations]  # pow takes a negative exponent: the inverse
    assert np.array_equal(cells[0], pkg.api.fr_cell(x)) and np.array_equal(cells[0], cells[4])
    assert pkg.api.rotated_points(1, 10, []).shape == (0, 32)
    with pytest.raises(ValueError):
        pkg.api.rotated_points(1, 29, [0])


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.OPEN_LIB_PATH, oc.launched())
    assert len(oc.launched()) == 9
    for name, words in (("test_gpu_open_columns.py", ("oc.SHAPES", "oc.STORE_MODES", "oc.points")), ("test_gpu_open_reach.py", ("oc.REACH_K",)),
                        ("test_gpu_open_chain.py", ("oc.CHAIN",))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"))
    table = cl.resource_table(code_object, columns)  # no scratch, no VGPR spills, at most 256 unified registers
    assert set(table) == oc.launched(), sorted(table)
    for name, row in table.items():
        assert row["global_atomics"] == 0, (name, row)  # every output word is stored, never added to
        assert row["mad_u64"] >= 2 * 64, (name, row)    # every kernel multiplies in the field: a product is 2 x 8 x 8 limb products
        if any(k in name for k in MEETING):
            assert row["static_lds"] > 0 and row["barriers"] >= 1, (name, row)
        else:  # a thread of the powers and of the fold kernel meets no other
            assert row["static_lds"] == 0 and row["barriers"] == 0, (name, row)
        if "scan" in name:
            assert row["global_stores"] == 8, (name, row)  # a lane's four cells, two 16-byte pieces each
        if "fold" in name:
            assert row["global_stores"] == 2, (name, row)
    cl.assert_tracked(table, TABLE)
