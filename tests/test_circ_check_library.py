"""libaesw_circ.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), holds gfx950 code, exports every function include/aesw_circ.h declares, and the Python face
    (Context.check_circuits) is there;
  * every __global__ instantiation in it is launched by the GPU sweep (tests/circ_check_cases.py), and that list names
    nothing else: the separate library is no way round "no kernel ships unswept";
  * its code object: no scratch, no VGPR spills, at most 256 unified registers (twelve waves per CU, what check_kernel runs
    at), compared with the tracked table profiles/isa_resources_circ.json.  Regenerate that table on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_circ_check_library.py;
  * libaesw.so is not touched: it holds no circ_check kernel and does not export the new entry point (its own kernel set and
    ISA table are pinned by the existing tests)."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

import circ_check_cases as ccc
from isa_extract import extract, needs_llvm, short as _short
from test_circuits_coverage import all_kernels

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "profiles" / "isa_resources_circ.json"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aesw_circ.h").read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(aesw_circ_\w+)\s*\(", text)))


def _nm(path, *flags):
    return subprocess.run(["nm", *flags, str(path)], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    lib = pkg.api.CIRC_LIB_PATH
    assert lib.name == "libaesw_circ.so" and lib.parent == pkg.api.LIB_PATH.parent and lib.exists()
    declared = _declared()
    assert "aesw_circ_check_witness_device" in declared and len(declared) >= 2, declared
    exported = {line.split()[-1] for line in _nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert not [f for f in declared if f not in exported], (declared, sorted(exported)[:20])
    loaded = pkg.api.load_circ_library()
    for f in declared:
        assert f in pkg.api.CIRC_SYMBOLS and getattr(loaded, f) is not None, f
    assert callable(pkg.Context.check_circuits)
    # it takes libaesw.so's contexts: NEEDED libaesw.so, found next to it
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn


def test_the_product_library_is_left_alone(pkg):
    text = _nm(pkg.api.LIB_PATH, "-C")
    assert "circ_check_kernel" not in text and "aesw_circ_check_witness_device" not in text
    assert not [ln for ln in (ROOT / "include" / "aesw.h").read_text().splitlines() if "aesw_circ_check" in ln]


def test_every_kernel_of_the_library_is_swept_and_the_list_names_nothing_else(pkg):
    lib = {"%s::%s" % (ns, name) if ns else name for ns, name in all_kernels(_nm(pkg.api.CIRC_LIB_PATH, "-C"))}
    assert lib == ccc.launched(), (sorted(lib), sorted(ccc.launched()))
    assert ccc.launched() == {"aesw_circ::circ_check_kernel<0>", "aesw_circ::circ_check_kernel<1>", "aesw_circ::circ_report_init_kernel"}
    # the GPU sweep really runs over that list
    src = (ROOT / "tests" / "test_gpu_circ_check.py").read_text()
    assert "ccc.LAYOUTS" in src and "ccc.SHAPES" in src


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    co = extract(pkg.api.CIRC_LIB_PATH, tmp_path_factory.mktemp("isa_circ"))
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
        # the offsets are searched with scalar loads (the search runs once per block and wave)
        if "circ_check_kernel" in short:
            assert any(t.startswith("s_load_dwordx2") for t in ins[50:]), "%s: the circuit search has no scalar load" % short
        table[short] = {
            "vgpr": k[".vgpr_count"], "agpr": k.get(".agpr_count", 0), "sgpr": k[".sgpr_count"],
            "sgpr_spill": k.get(".sgpr_spill_count", 0), "static_lds": k[".group_segment_fixed_size"],
            "instructions": len(ins),
            "global_loads": sum(1 for t in ins if t.startswith("global_load_")),
            "scalar_loads_x2": sum(1 for t in ins if t.startswith("s_load_dwordx2")),
            "global_stores": sum(1 for t in ins if t.startswith("global_store_")),
            "global_atomics": sum(1 for t in ins if t.startswith("global_atomic_")),
        }
    assert set(table) == ccc.launched(), sorted(table)
    table = dict(sorted(table.items()))
    if os.environ.get("AESW_UPDATE_ISA_JSON"):
        TABLE.write_text(json.dumps(table, indent=1) + "\n")
    assert TABLE.exists(), "profiles/isa_resources_circ.json is missing: run with AESW_UPDATE_ISA_JSON=1 and commit it"
    tracked = json.loads(TABLE.read_text())
    assert tracked == table, ("the built kernels differ from profiles/isa_resources_circ.json (regenerate it with "
                              "AESW_UPDATE_ISA_JSON=1 and commit the diff if the change is intended): %r" % (table,))
