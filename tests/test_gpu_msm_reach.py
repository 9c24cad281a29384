"""What the shapes of tests/test_gpu_msm_columns.py never reach: a workgroup of the bucket kernel that walks more than one chunk,
and a reduce that sums more than one slice, both under the library's OWN slice rule (slices = 0).  The smallest such k is read
from the rules through the library -- aesw_msm_chunk_rows and aesw_msm_slices -- not written down here; with the committed values
it is 14.  The expectation is the commitment by known logarithms: one affine addition a basis point and one scalar
multiplication a column."""
import numpy as np
import pytest

import guarded as G
import msm_cases as mc
import msm_model as mm

pytestmark = pytest.mark.gpu


def reach_k(lib, kind):
    """the smallest k whose automatic slices are more than one and hold more than one chunk each"""
    chunk = int(lib.aesw_msm_chunk_rows())
    for k in range(10, 21):
        slices = int(lib.aesw_msm_slices(k, 1, kind, 0))
        rows = -(-(-(-(1 << k) // slices)) // 16) * 16
        if slices > 1 and rows > chunk:
            return k, slices
    raise AssertionError("no k up to 20 reaches two slices of two chunks")


@pytest.mark.parametrize("kind", (mc.FR, mc.BYTES), ids=mc.kind_name)
def test_two_chunks_a_workgroup_and_two_slices_a_bucket(pkg, ctx, kind):
    import torch
    lib = pkg.api.load_msm_library()
    k, slices = reach_k(lib, kind)
    assert k <= 16, "the model's basis costs 2^k affine additions"
    n = 1 << k
    values = mm.seeded_scalars(n, 0x7265 + k) if kind == mc.FR else [int(v) for v in np.random.default_rng(0x7265 + k).integers(0, 256, n)]
    scalars = mc.scalar_bytes(kind, values).reshape((1, n, 32) if kind == mc.FR else (1, n))
    arena = G.DeviceArena()
    d_scalars = arena.out("scalars", scalars.size, scalars.shape)
    d_scalars.copy_(torch.from_numpy(scalars).to(d_scalars.device))
    ws = arena.out("ws", int(lib.aesw_msm_workspace_bytes(k, 1, kind, 0)))
    got = ctx.commit_columns(d_scalars, torch.from_numpy(mc.basis_cells(k)).cuda(), out=arena.out("out", 64, (1, 64)), _workspace=ws)
    arena.check()
    G.assert_bytes("k=%d %s, %d slices" % (k, mc.kind_name(kind), slices), got.cpu().numpy()[0], mm.to_points([mm.known_commit(values)])[0])
