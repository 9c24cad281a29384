"""examples/aesw_circ_check.c: the many-circuit batch made and certified from plain C, linked against both libraries."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_certifies_a_batch_and_names_the_changed_byte(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_circ_check"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_circ_check.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_circ", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for args in (["14", "1", "64"], ["16", "3", "5"]):
        out = subprocess.run([str(exe)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0, out.stdout
        assert "0 lookup, 0 copy, 0 gate, 0 literal, 0 offset failures" in out.stdout and out.stdout.rstrip().endswith("ok"), out.stdout
        assert "of circuit 2), lookup, row 40" in out.stdout, out.stdout
