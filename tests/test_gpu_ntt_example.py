"""examples/aesw_ntt.c on the GPU: two columns to their coefficients, onto the extended coset, back in place, and to Lagrange form
again, from plain C with no Python in the process.  The example checks the round trips, the zero padding and the constant column
itself; here its figures are held against the shape."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_goes_round_and_comes_back(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_ntt"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_ntt.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_ntt", "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k in (12, 17):
        out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        assert "2 columns of 2^%d cells: coefficients, 2^%d evaluations on the coset (zeta_sel 1), %d coefficients back with %d zero cells behind them" % (
            k, k + 2, 2 << k, 6 << k) in out.stdout
    assert subprocess.run([str(exe), "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
