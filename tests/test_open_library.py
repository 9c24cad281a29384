"""libaesw_open.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_open_ functions include/aesw_open.h declares, api.OPEN_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one; it is the one entry of
    _build.OPENING_LIBRARIES, a sixth table that none of the five older name functions lists and library_entry() knows;
  * a Group refuses; a missing path says how to build it; rotated_points is x * omega_k^r in cells;
  * every __global__ in it is launched by the GPU tests (tests/open_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic in any kernel, the field products as 64-bit multiply-adds, at most 256
    unified registers, LDS and barriers only in the kernels whose waves meet; compared with the tracked table
    profiles/isa_resources_open.json (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_open_library.py);
  * the other libraries and their headers carry none of the new symbols, and the header names no other library."""
import importlib.util
import subprocess

import numpy as np
import pytest

import check_library as cl
import ntt_model as nm
import open_cases as oc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_open.json"
code_object = cl.code_object_fixture("OPEN_LIB_PATH")
DECLARED = ["aesw_open_divide_device", "aesw_open_evaluate_device", "aesw_open_fold_device", "aesw_open_workspace_bytes"]
OTHERS = ("LIB_PATH", "CIRC_LIB_PATH", "COLS_LIB_PATH", "VALS_LIB_PATH", "ACC_LIB_PATH", "VACC_LIB_PATH", "MULT_LIB_PATH", "PERM_LIB_PATH", "THETA_LIB_PATH",
          "GRAND_LIB_PATH", "SIGMA_LIB_PATH", "NTT_LIB_PATH", "QUOT_LIB_PATH", "HOST_LIB_PATH")
OTHER_LIBRARIES_IN_WORDS = ("aesw_ntt", "aesw_quot", "aesw_grand", "aesw_sigma", "aesw_theta", "aesw_perm", "aesw_mult", "aesw_acc", "aesw_vacc", "aesw_vals",
                            "aesw_cols", "aesw_circ")
METHODS = ("evaluate_columns", "fold_columns", "divide_columns")
MEETING = ("open_chunk_kernel", "open_carry_kernel", "open_scan_kernel")  # the kernels whose waves meet through LDS


def _build_module():
    spec = importlib.util.spec_from_file_location("b", cl.ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.OPEN_LIB_PATH
    assert lib.name == "libaesw_open.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = cl.declared("aesw_open.h", "aesw_open_")
    assert decl == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    loaded = api.load_open_library()
    assert api.load_open_library() is loaded
    assert sorted(api.OPEN_SYMBOLS) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES["open"] == (lib, api.OPEN_SYMBOLS, api._NO_FALLBACK)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    others = ("libaesw_acc", "libaesw_vacc", "libaesw_mult", "libaesw_perm", "libaesw_theta", "libaesw_grand", "libaesw_sigma", "libaesw_ntt", "libaesw_quot",
              "libaesw_vals", "libaesw_circ", "libaesw_cols", "libaesw_host")
    assert not [s for s in others if s in dyn], dyn
    source = cl.ROOT / "halo2-aes_amd" / "csrc" / "open" / "aesw_open.hip"  # one level below csrc/, as every satellite's
    assert "namespace aesw_open {" in source.read_text() and '#include "../aesw_fr_dev.h"' in source.read_text()
    for name in METHODS:
        assert callable(getattr(api.Context, name)), name
    header = (cl.ROOT / "include" / "aesw_open.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "NOT PINNED" in header and "NON-CANONICAL" in header
    assert not [w for w in OTHER_LIBRARIES_IN_WORDS if w in header]


def test_the_entry_is_a_sixth_table_and_the_five_name_functions_stay_what_they_are():
    b = _build_module()
    assert list(b.OPENING_LIBRARIES) == ["open"] == b.opening_library_names() and b.OPEN_LIB == b.PKG / "libaesw_open.so"
    assert b.library_names() == list(b.SATELLITES) + list(b.FIELD_LIBRARIES) + list(b.ARGUMENT_LIBRARIES) and "open" not in b.library_names()
    assert b.domain_library_names() == ["ntt"] == list(b.DOMAIN_LIBRARIES) and b.quotient_library_names() == ["quot"] == list(b.QUOTIENT_LIBRARIES)
    assert list(b.SATELLITES) == ["circ", "cols", "vals", "acc", "perm", "vacc", "mult"] and list(b.FIELD_LIBRARIES) == ["theta"]
    assert list(b.ARGUMENT_LIBRARIES) == ["grand", "sigma"]
    sources, headers, public = b.library_entry("open")
    assert sources[0].parent.name == "open" and public.name == "aesw_open.h" and [h.name for h in headers] == ["aesw_fr.h", "aesw_open.h"]
    assert all(h.exists() for h in headers)
    assert b.library_entry("quot")[2].name == "aesw_quot.h" and b.library_entry("mult")[2].name == "aesw_mult.h"
    with pytest.raises(KeyError):
        b.library_entry("nowhere")
    entry = (cl.ROOT / "__graft_entry__.py").read_text()
    assert entry.count("b.quotient_library_names() + b.opening_library_names()") == 2  # built last, loaded last


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    missing = tmp_path / "nowhere" / pkg.api.OPEN_LIB_PATH.name
    with pytest.raises(FileNotFoundError) as e:
        pkg.api.load_open_library(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def test_the_other_libraries_are_left_alone(pkg):
    for other in OTHERS:
        text = cl.nm(getattr(pkg.api, other), "-C")
        assert "aesw_open" not in text and "open_chunk_kernel" not in text and "open_fold_kernel" not in text, other
    for header in sorted((cl.ROOT / "include").glob("*.h")):
        if header.name != "aesw_open.h":
            assert "aesw_open" not in header.read_text(), header.name


def test_a_group_refuses(pkg):
    for name in METHODS:
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, name)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


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
