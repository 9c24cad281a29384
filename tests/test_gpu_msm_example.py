"""examples/aesw_msm.c on the GPU: a basis from plain coordinates, checked; five columns committed as bytes and as cells, from plain
C with no Python in the process.  The example checks what bytes alone can say -- the identity, G itself, G + (-G), G + G against
2 * G, cells against bytes, the report of a point off the curve -- itself; here its figures are held against the shape."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_commits_bytes_and_cells(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_msm"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_msm.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_msm", "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    lib = pkg.api.load_msm_library()
    for k in (10, 16):
        out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        assert "5 columns of 2^%d rows as bytes and as cells: 10 commitments, %d slices a byte column and %d a column of cells, chunks of %d rows" % (
            k, lib.aesw_msm_slices(k, 5, 1, 0), lib.aesw_msm_slices(k, 5, 0, 0), lib.aesw_msm_chunk_rows()) in out.stdout
    assert subprocess.run([str(exe), "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
