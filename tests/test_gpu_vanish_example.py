"""examples/aesw_vanish.c on the GPU: the quotient of one small shape folded segment by segment from plain C with no Python in the
process, in place and from buffer to buffer, and held by the example itself against tests/golden/vanish_example_k10.bin -- the cells
csrc/aesw_vanish.h's own fold gives on the CPU.  The golden file is held here too: the example writes its input, tests/vanish_driver.cpp
folds it, and the bytes are the file's."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "vanish_example_k10.bin"


def test_the_plain_c_example_folds_the_quotient_segment_by_segment(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_vanish"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_vanish.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_vanish", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe), str(GOLDEN), str(tmp_path / "in.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
    assert "40 columns of 2^12 cells folded in 5 segments: 4096 cells, " in out.stdout
    moved = int(out.stdout.split("4096 cells, ")[1].split()[0])
    assert moved >= 4090, out.stdout  # y multiplies every row's fold; a cell stays only by a chance of 2^-254
    # a wrong golden file is noticed
    wrong = tmp_path / "wrong.bin"
    wrong.write_bytes(bytes([GOLDEN.read_bytes()[0] ^ 1]) + GOLDEN.read_bytes()[1:])
    assert subprocess.run([str(exe), str(wrong)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 5
    assert subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
    # the golden file is what the header's fold gives for the example's input on the CPU
    driver = tmp_path / "vanish_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", str(ROOT / "halo2-aes_amd" / "csrc"), str(ROOT / "tests" / "vanish_driver.cpp"), "-o", str(driver)], check=True)
    subprocess.run([str(driver), "run", "10", "12", "1", "1", "3", "1018", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    assert (tmp_path / "out.bin").read_bytes() == GOLDEN.read_bytes() and len(GOLDEN.read_bytes()) == 4096 * 32
