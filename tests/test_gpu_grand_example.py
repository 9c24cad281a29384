"""examples/aesw_grand.c on the GPU: witness -> multiplicities -> permuted indices -> input indices -> theta -> compressed tables
-> beta, gamma -> inverse table -> Z of every argument, from plain C with no Python in the process.  The example checks Z[0], the
closing cells and the report itself; here its figures are held against the selectors."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_builds_z_and_every_argument_closes(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_grand"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_grand.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_grand", "-laesw_theta", "-laesw_perm", "-laesw_mult",
                    "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    k, n_sets = 17, 1
    out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
    n, u = pkg.block_capacity(k, n_sets), (1 << k) - 6
    sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
    lines = re.findall(r"tag (\d+): Z closes at row (\d+), (\d+) rows move it", out.stdout)
    assert len(lines) == 5
    for line in lines:
        tag, row, moved = [int(v) for v in line]
        assert row == u and 0 < moved <= u and int(sel[tag - 1, :u].sum()) > 0, line  # the argument has lookups: Z is no constant column
    assert "%d blocks (K = %d, N = %d), %d lookups, %d usable rows: Z of 5 arguments, 0 zero terms, 0 open" % (n, k, n_sets, 400 + 1056 * n, u) in out.stdout
    assert subprocess.run([str(exe), "16"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1  # no room for the table
