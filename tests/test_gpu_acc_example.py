"""examples/aesw_acc.c: one circuit generated in four chunks into the same slab buffers and counted chunk by chunk, from plain C,
linked against libaesw_acc.so and libaesw.so."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_prints_the_selector_popcounts(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_acc"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_acc.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_acc", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    for k, n_sets in ((14, 3), (13, 2)):
        out = subprocess.run([str(exe), str(k), str(n_sets)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        n = pkg.block_capacity(k, n_sets)
        sel, _fixed = pkg.assemble_selectors(k, n_sets, n)
        lines = re.findall(r"set (\d+): range (\d+) xor (\d+) sbox (\d+) mul2 (\d+) mul3 (\d+)", out.stdout)
        assert len(lines) == n_sets
        for line in lines:
            s, *sums = [int(v) for v in line]
            assert sums == [int(sel[5 * s + i].sum()) for i in range(5)], line
        assert "%d blocks in 4 chunks" % n in out.stdout and "%d lookups, 0 misses" % (400 + 1056 * n) in out.stdout, out.stdout
