"""examples/aesw_theta.c on the GPU: witness -> multiplicities -> permuted indices -> input indices -> theta -> compressed tables
-> the four columns of every argument as Fr cells, from plain C with no Python in the process.  The example checks plookup's
two relations on the Fr bytes itself; here its figures are held against the selectors."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_compresses_and_checks_the_relations(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_theta"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_theta.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_theta", "-laesw_perm", "-laesw_mult", "-laesw",
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    k, n_sets = 17, 1
    out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
    n, u = pkg.block_capacity(k, n_sets), (1 << k) - 6
    sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
    lines = re.findall(r"tag (\d+): (\d+) enabled rows below (\d+), table (\d+)", out.stdout)
    assert len(lines) == 5
    for line in lines:
        tag, enabled, below, table = [int(v) for v in line]
        assert below == u and enabled == int(sel[tag - 1, :u].sum()) and table == {1: 0, 2: 2}.get(tag, 1), line  # selector i of a set is tag i + 1
    assert "%d blocks (K = %d, N = %d), %d lookups, %d usable rows: 4 columns of 5 arguments as Fr cells" % (n, k, n_sets, 400 + 1056 * n, u) in out.stdout
    assert subprocess.run([str(exe), "16"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1  # no room for the table
