"""examples/aesw_open.c on the GPU: two coefficient columns at three points, divided by (X - z) out of place and by X in place, and
folded under v column by column, from plain C with no Python in the process.  The example checks what bytes alone can say -- the
value at 0, the remainder against the evaluation, the shift of a division by X, the fold under 0 -- itself; here its figures are
held against the shape."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_evaluates_divides_and_folds(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_open"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_open.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_open", "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k in (11, 17):
        out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        assert "2 columns of 2^%d coefficients: 6 evaluations, %d quotient coefficients at z and %d at 0 in place, 2 columns folded under v into %d cells" % (
            k, 2 << k, 2 << k, 1 << k) in out.stdout
    assert subprocess.run([str(exe), "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
