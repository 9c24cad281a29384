"""libaesw_open.so where the sweep of tests/test_gpu_open_columns.py never reaches: the second turn of the carry kernel.

oc.REACH_K = 19 is the smallest k whose column has more chunks (512 of 1 024 cells) than the carry kernel scans a turn (256): the
value of the upper turn enters the lower one as its running cell, and a chunk's carry-in crosses the turn.  One column, one seeded
point, on poisoned, guard-banded buffers: every cell of q, the remainder and the evaluation against ONE run of the model (about a
second of Python), which also gives the evaluation -- it is the remainder."""
import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import open_cases as oc
import open_model as om

pytestmark = pytest.mark.gpu


def test_the_second_turn_of_the_carry_is_the_models(pkg, ctx):
    import torch
    k = oc.REACH_K
    coeff = nm.seeded_values(1 << k, 0x7265)
    z = nm.seeded_values(1, 0x727a)[0]
    q, rem = om.divide(coeff, z)
    cells = nm.to_cells(coeff).reshape(1, 1 << k, 32)
    lib = pkg.api.load_open_library()
    arena = G.DeviceArena()
    d_coeff = arena.out("coeff", cells.size, cells.shape)
    d_coeff.copy_(torch.from_numpy(cells).to(d_coeff.device))
    ws = lambda: arena.out("ws", int(lib.aesw_open_workspace_bytes(k, 1, 1)))  # noqa: E731
    value = ctx.evaluate_columns(d_coeff, k, z, out=arena.out("value", 32, (1, 1, 32)), _workspace=ws())
    quot, got_rem = ctx.divide_columns(d_coeff, k, z, out=arena.out("quot", cells.size, cells.shape), _rem=arena.out("rem", 32, (1, 32)), _workspace=ws())
    arena.check()
    G.assert_bytes("the quotient at k = %d" % k, quot.cpu().numpy(), nm.to_cells(q))
    G.assert_bytes("the remainder", got_rem.cpu().numpy(), nm.to_cells([rem]))
    G.assert_bytes("the evaluation", value.cpu().numpy(), nm.to_cells([rem]))
    G.assert_bytes("the input is left alone", d_coeff.cpu().numpy(), cells)
    assert q[-1] == 0 and q[-2] == coeff[-1] and np.any(quot[0, (1 << k) - 2].cpu().numpy())
