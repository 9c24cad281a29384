"""examples/aesw_transcript.c on the GPU: a basis, two byte columns committed, the commitments written into the transcript, theta
squeezed and handed as a device pointer to the table compression -- from plain C with no Python in the process, one stream and one
wait.  Its output -- the proof's hex, theta's cell, the count words -- is held against tests/transcript_model.py: the columns commit
to G and to 3 G."""
import subprocess
from pathlib import Path

import pytest

import msm_model as mm
import transcript_model as tm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_the_plain_c_example_prints_the_models_proof_and_theta(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_transcript"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_transcript.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_transcript", "-laesw_msm", "-laesw_theta", "-laesw",
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    model = tm.Transcript().write_points([mm.GENERATOR, mm.mul(3, mm.GENERATOR)])
    proof, theta = model.proof.hex(), tm.challenge_cell(model.squeeze()).tobytes().hex()
    for k in (10, 11):
        out = subprocess.run([str(exe), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        lines = out.stdout.splitlines()
        assert "proof " + proof in lines and "theta " + theta in lines, out.stdout
        assert "status proof_bytes 64 proof_missed 0 identities 0 points 2" in lines and "table cells %d noncanonical 0" % (3 * pkg.TABLE_ROWS) in lines, out.stdout
    assert subprocess.run([str(exe), "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 1
