"""examples/aesw_sigma.c on the GPU: witness -> byte columns -> sigma, sources, the fixed column and the power tables -> beta, gamma
-> Z of both sets, from plain C with no Python in the process.  The example checks Z_s[0], the closing cells and the report itself;
here its figures are held against the mapping."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_builds_z_and_the_argument_closes(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_sigma"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_sigma.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_sigma", "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    k, n_sets = 17, 1
    out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
    n, u = pkg.block_capacity(k, n_sets), (1 << k) - 6
    mapping = pkg.api.permutation_mapping(k, n_sets, n)
    moved = int((mapping.reshape(-1) != np.arange(mapping.size)).sum())
    assert moved > 1000 * n
    assert re.findall(r"set (\d+): columns (\d+) ... (\d+), Z closes at row (\d+)", out.stdout) == [("0", "0", "2", str(u)), ("1", "3", "4", str(u))]
    assert "%d blocks (K = %d, N = %d), 5 columns, %d cells moved by sigma, %d usable rows: Z of 2 sets, 0 zero terms, 0 out of range, closed" % (n, k, n_sets, moved, u) \
        in out.stdout
    assert subprocess.run([str(exe), "11"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
