"""examples/aesw_shplonk.c on the GPU: one column opened at two points in one set -- N_0, h, L' and W -- from plain C with no Python in
the process.  The example checks what bytes alone can say itself (zero remainders, a clean report, the degree dropping by two in h
and by one in W, z_0 = 1, and a report that names set 0 once the evaluations are swapped); here its figures are held against the shape."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_opens_a_column_at_two_points(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_shplonk"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_shplonk.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_shplonk", "-laesw_open", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k in (11, 17):
        out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        assert "1 column of 2^%d coefficients at 2 points: h and W of %d coefficients each, report 0 0, with the evaluations swapped 1 0" % (k, 1 << k) in out.stdout
    assert subprocess.run([str(exe), "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
