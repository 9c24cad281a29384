"""libaesw_cols.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_cols.h declares, its NEEDED entry is
    libaesw.so via $ORIGIN, and the Python face (Context.check_columns) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/cols_check_cases.py), and that list names
    nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, compared with the tracked table
    profiles/isa_resources_cols.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_cols_check_library.py;
  * libaesw.so and libaesw_circ.so carry none of the new symbols."""
import json
import os
import re
import subprocess
from pathlib import Path

import cols_check_cases as ccs
from isa_extract import extract, needs_llvm, short as _short
from test_circ_check_library import _nm
from test_circuits_coverage import all_kernels

import pytest

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "profiles" / "isa_resources_cols.json"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aesw_cols.h").read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(aesw_cols_\w+)\s*\(", text)))


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    lib = pkg.api.COLS_LIB_PATH
    assert lib.name == "libaesw_cols.so" and lib.parent == pkg.api.LIB_PATH.parent and lib.exists()
    declared = _declared()
    assert "aesw_cols_check_device" in declared and "aesw_cols_cell_index" in declared and len(declared) >= 5, declared
    exported = {line.split()[-1] for line in _nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert not [f for f in declared if f not in exported], (declared, sorted(exported)[:20])
    loaded = pkg.api.load_cols_library()
    for f in declared:
        assert f in pkg.api.COLS_SYMBOLS and getattr(loaded, f) is not None, f
    assert sorted(pkg.api.COLS_SYMBOLS) == declared
    assert callable(pkg.Context.check_columns)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    # the sources live one level below csrc/, which keeps holding exactly the sources of libaesw.so
    assert (ROOT / "halo2-aes_amd" / "csrc" / "cols" / "aesw_cols_check.hip").exists()


def test_the_other_libraries_are_left_alone(pkg):
    for other in (pkg.api.LIB_PATH, pkg.api.CIRC_LIB_PATH):
        text = _nm(other, "-C")
        assert "cols_check_kernel" not in text and "aesw_cols_" not in text, other
    for header in ("aesw.h", "aesw_circ.h"):
        assert "aesw_cols" not in (ROOT / "include" / header).read_text()


def test_the_cell_index_helper(pkg):
    lib = pkg.api.load_cols_library()
    assert lib.aesw_cols_cell_index(14, 1, 0, 0, 0) == 0
    assert lib.aesw_cols_cell_index(14, 1, 3, 2, 77) == ((3 * 4 + 2) << 14) + 77
    assert lib.aesw_cols_cell_index(30, 1024, 5, 3072, (1 << 30) - 1) == ((5 * 3073 + 3072) << 30) + (1 << 30) - 1


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    lib = {"%s::%s" % (ns, name) if ns else name for ns, name in all_kernels(_nm(pkg.api.COLS_LIB_PATH, "-C"))}
    assert lib == ccs.launched(), (sorted(lib), sorted(ccs.launched()))
    assert ccs.launched() == {"aesw_cols::cols_check_kernel<false>", "aesw_cols::cols_check_kernel<true>", "aesw_cols::cols_report_init_kernel"}
    src = (ROOT / "tests" / "test_gpu_cols_check.py").read_text()
    assert "ccs.FORMS" in src and "ccs.SHAPES" in src


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    co = extract(pkg.api.COLS_LIB_PATH, tmp_path_factory.mktemp("isa_cols"))
    assert co["target"].endswith("gfx950"), co["target"]
    return co


@needs_llvm
def test_gfx950_code_without_scratch_or_spills_and_the_tracked_table(code_object):
    table = {}
    for name, k in code_object["meta"].items():
        ins = code_object["funcs"].get(name, [])
        short = _short(code_object["demangled"][name])
        assert k[".private_segment_fixed_size"] == 0, "%s uses %d B of scratch" % (short, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0, "%s spills VGPRs" % short
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 256, (short, k[".vgpr_count"], k.get(".agpr_count", 0))
        if "cols_check_kernel" in short:  # the circuit search and the sweep's offsets run on scalar loads
            assert any(t.startswith("s_load_dwordx2") or t.startswith("s_load_dwordx4") for t in ins[50:]), "%s: no scalar load of the offsets" % short
        table[short] = {
            "vgpr": k[".vgpr_count"], "agpr": k.get(".agpr_count", 0), "sgpr": k[".sgpr_count"],
            "sgpr_spill": k.get(".sgpr_spill_count", 0), "static_lds": k[".group_segment_fixed_size"],
            "instructions": len(ins),
            "global_loads": sum(1 for t in ins if t.startswith("global_load_")),
            "global_stores": sum(1 for t in ins if t.startswith("global_store_")),
            "global_atomics": sum(1 for t in ins if t.startswith("global_atomic_")),
        }
    assert set(table) == ccs.launched(), sorted(table)
    table = dict(sorted(table.items()))
    if os.environ.get("AESW_UPDATE_ISA_JSON"):
        TABLE.write_text(json.dumps(table, indent=1) + "\n")
    assert TABLE.exists(), "profiles/isa_resources_cols.json is missing: run with AESW_UPDATE_ISA_JSON=1 and commit it"
    tracked = json.loads(TABLE.read_text())
    assert tracked == table, ("the built kernels differ from profiles/isa_resources_cols.json (regenerate it with "
                              "AESW_UPDATE_ISA_JSON=1 and commit the diff if the change is intended): %r" % (table,))
