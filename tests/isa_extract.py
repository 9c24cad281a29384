"""The gfx950 code object inside one of the built libraries, for the CPU tests that look at the compiled kernels
(test_isa_lint.py: libaesw.so; through check_library.py test_circ_check_library.py: libaesw_circ.so,
test_cols_check_library.py: libaesw_cols.so and test_vals_check_library.py: libaesw_vals.so):
objcopy takes the fat binary out of the library, clang-offload-bundler the gfx950 object out of that, llvm-objdump and
llvm-readelf give its disassembly and kernel metadata.  Each test compares what it finds with its own tracked table."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import yaml

LLVM = Path("/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

needs_llvm = pytest.mark.skipif(not (LLVM / "llvm-objdump").exists() or shutil.which("objcopy") is None or shutil.which("c++filt") is None,
                                reason="needs the ROCm LLVM tools, objcopy and c++filt")


def extract(lib, workdir):
    """{"target": the code object's target, "meta": kernel metadata by mangled name, "demangled": mangled -> demangled name,
    "funcs": mangled name -> its instructions ("mnemonic operands", in order)} of the library at `lib`; files go to `workdir`."""
    fat, co = Path(workdir) / "fat.bin", Path(workdir) / "k.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + str(fat),
                    "--output=" + str(co), "--unbundle"], check=True)
    asm = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(co)], stdout=subprocess.PIPE, text=True, check=True).stdout
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], stdout=subprocess.PIPE, text=True, check=True).stdout
    meta = yaml.safe_load(notes[notes.index("---"):notes.index("...", notes.index("---"))])
    names = [k[".name"] for k in meta["amdhsa.kernels"]]
    dem = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    # per-function instruction lists: "<mangled>:" labels, then "\tmnemonic operands // addr: encoding"
    funcs, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return {"target": meta["amdhsa.target"], "meta": {k[".name"]: k for k in meta["amdhsa.kernels"]}, "demangled": dict(zip(names, dem)),
            "funcs": funcs}


def short(demangled, drop=""):
    """aesw::encrypt_kernel<1, true, 0, true, 2>(aesw::EncParams) -> aesw::encrypt_kernel<1,true,0,true,2>, without the
    namespace prefix `drop` where one is given"""
    s = re.sub(r"\(.*\)$", "", demangled.replace("void ", ""))
    if drop:
        s = s.replace(drop, "")
    return s.replace(", ", ",")
