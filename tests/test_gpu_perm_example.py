"""examples/aesw_perm.c on the GPU: witness -> multiplicities -> permuted columns -> gathered cells from plain C, with no Python
in the process.  The example checks plookup's relations itself; here its figures are held against the selectors."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_arranges_and_gathers(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_perm"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_perm.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_perm", "-laesw_acc", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    k, n_sets = 17, 2
    out = subprocess.run([str(exe), str(k), str(n_sets)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
    n, u = pkg.block_capacity(k, n_sets), (1 << k) - 6
    sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
    lines = re.findall(r"set (\d+) tag (\d+): (\d+) lookups, (\d+) rows of the all-zero run", out.stdout)
    assert len(lines) == 5 * n_sets
    for line in lines:
        s, tag, lookups, zeros = [int(v) for v in line]
        assert lookups == int(sel[5 * s + tag - 1].sum()) and zeros == u - lookups, line  # selector i of a set is tag i + 1
    assert "%d blocks (K = %d, N = %d), %d usable rows: %d arguments arranged" % (n, k, n_sets, u, 5 * n_sets) in out.stdout, out.stdout
    assert subprocess.run([str(exe), "16"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1  # no room for the table
