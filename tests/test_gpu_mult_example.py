"""examples/aesw_mult.c: the lookup multiplicities of a few circuits counted from plain C, linked against both libraries."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_prints_the_selector_popcounts(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_mult"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_mult.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_mult", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k, n_sets, nc in ((13, 3, 3), (14, 1, 70)):  # the second shape takes the other form by default
        out = subprocess.run([str(exe), str(k), str(n_sets), str(nc)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        cap = pkg.block_capacity(k, n_sets)
        counts = [cap // 2 if c == 1 else cap for c in range(nc)]
        lines = re.findall(r"circuit (\d+) set (\d+): range (\d+) xor (\d+) sbox (\d+) mul2 (\d+) mul3 (\d+)", out.stdout)
        assert len(lines) == nc * n_sets
        for line in lines:
            c, s, *sums = [int(v) for v in line]
            sel, _fixed = pkg.assemble_selectors(k, n_sets, counts[c])
            assert sums == [int(sel[5 * s + i].sum()) for i in range(5)], line
        assert "%d lookups, 0 misses" % (400 * nc + 1056 * sum(counts)) in out.stdout, out.stdout
    assert pkg.api.load_mult_library().aesw_mult_default_form(13, 3, 3) != pkg.api.load_mult_library().aesw_mult_default_form(14, 1, 70)
