"""libaesw_vals.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_vals.h declares, its NEEDED entry is
    libaesw.so via $ORIGIN, and the Python face (Context.check_values) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/vals_check_cases.py), and that list names
    nothing else;
  * its code object: no scratch, no VGPR spills, at most 256 unified registers, compared with the tracked table
    profiles/isa_resources_vals.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_vals_check_library.py;
  * the three other libraries and their headers carry none of the new symbols."""
import json
import os
import re
import subprocess
from pathlib import Path

import vals_check_cases as vcs
from isa_extract import extract, needs_llvm, short as _short
from test_circ_check_library import _nm
from test_circuits_coverage import all_kernels

import pytest

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "profiles" / "isa_resources_vals.json"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aesw_vals.h").read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(aesw_vals_\w+)\s*\(", text)))


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    lib = pkg.api.VALS_LIB_PATH
    assert lib.name == "libaesw_vals.so" and lib.parent == pkg.api.LIB_PATH.parent and lib.exists()
    declared = _declared()
    assert {"aesw_vals_check_device", "aesw_vals_check_rows", "aesw_vals_check_table", "aesw_vals_image_bytes"} <= set(declared), declared
    exported = {line.split()[-1] for line in _nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert not [f for f in declared if f not in exported], (declared, sorted(exported)[:20])
    assert sorted(f for f in exported if f.startswith("aesw_vals_")) == declared
    loaded = pkg.api.load_vals_library()
    for f in declared:
        assert f in pkg.api.VALS_SYMBOLS and getattr(loaded, f) is not None, f
    assert sorted(pkg.api.VALS_SYMBOLS) == declared
    assert callable(pkg.Context.check_values)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    # the sources live one level below csrc/, which keeps holding exactly the sources of libaesw.so
    assert (ROOT / "halo2-aes_amd" / "csrc" / "vals" / "aesw_vals_check.hip").exists()


def test_the_other_libraries_are_left_alone(pkg):
    for other in (pkg.api.LIB_PATH, pkg.api.CIRC_LIB_PATH, pkg.api.COLS_LIB_PATH):
        text = _nm(other, "-C")
        assert "vals_check_kernel" not in text and "aesw_vals" not in text, other
    for header in ("aesw.h", "aesw_circ.h", "aesw_cols.h"):
        text = (ROOT / "include" / header).read_text()
        assert "aesw_vals" not in text and "vals_check_kernel" not in text


def test_a_group_refuses_the_values_check(pkg):
    with pytest.raises(pkg.AeswError) as e:
        pkg.Group.check_values(None, None, None, None, None)
    assert e.value.status == pkg.api.ERR_INVALID_ARG


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    lib = {"%s::%s" % (ns, name) if ns else name for ns, name in all_kernels(_nm(pkg.api.VALS_LIB_PATH, "-C"))}
    assert lib == vcs.launched(), (sorted(lib), sorted(vcs.launched()))
    assert vcs.launched() == {"aesw_vals::vals_check_kernel<false>", "aesw_vals::vals_check_kernel<true>", "aesw_vals::vals_report_init_kernel"}
    src = (ROOT / "tests" / "test_gpu_vals_check.py").read_text()
    assert "vcs.KEY_MODES" in src and "vcs.SIZES" in src and "vcs.TABLE_SETS" in src


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    co = extract(pkg.api.VALS_LIB_PATH, tmp_path_factory.mktemp("isa_vals"))
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
        if "vals_check_kernel" in short:  # a block travels as 16-byte loads
            assert sum(1 for t in ins if t.startswith("global_load_dwordx4")) >= 4, "%s: no 16-byte loads" % short
        table[short] = {
            "vgpr": k[".vgpr_count"], "agpr": k.get(".agpr_count", 0), "sgpr": k[".sgpr_count"],
            "sgpr_spill": k.get(".sgpr_spill_count", 0), "static_lds": k[".group_segment_fixed_size"],
            "instructions": len(ins),
            "global_loads": sum(1 for t in ins if t.startswith("global_load_")),
            "global_stores": sum(1 for t in ins if t.startswith("global_store_")),
            "global_atomics": sum(1 for t in ins if t.startswith("global_atomic_")),
        }
    assert set(table) == vcs.launched(), sorted(table)
    table = dict(sorted(table.items()))
    if os.environ.get("AESW_UPDATE_ISA_JSON"):
        TABLE.write_text(json.dumps(table, indent=1) + "\n")
    assert TABLE.exists(), "profiles/isa_resources_vals.json is missing: run with AESW_UPDATE_ISA_JSON=1 and commit it"
    tracked = json.loads(TABLE.read_text())
    assert tracked == table, ("the built kernels differ from profiles/isa_resources_vals.json (regenerate it with "
                              "AESW_UPDATE_ISA_JSON=1 and commit the diff if the change is intended): %r" % (table,))
