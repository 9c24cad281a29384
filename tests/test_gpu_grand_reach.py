"""aesw_grand_product_device on the GPU where tests/test_gpu_grand_product.py never reaches (tests/grand_cases.py:
gc.MANY_CHUNKS): k = 19 and 2^18 + 3 rows, 257 chunks an argument, so that grand_carry_kernel's loop of 256 chunks a turn takes a
second turn, whose one chunk lies above the product of the whole first turn.  The columns are those of
tests/test_gpu_grand_product.py, seeded per argument, over 2^19 rows.  The device runs once, into poisoned, guard-banded outputs
(tests/guarded.py); each of the five arguments is then compared on its own with tests/grand_model.py in Python integers -- every
cell of Z from row 0 to row n_rows and the closing cell, byte for byte -- and a last test holds the report, the poison above row
n_rows and the guard bands.  The five closing products differ: a carry that leaks across arguments cannot hide."""
import numpy as np
import pytest

import grand_cases as gc
import grand_model as gm
import guarded as G
import test_gpu_grand_product as gp

pytestmark = pytest.mark.gpu
K, N_SETS, N_ROWS, PAD = gc.MANY_CHUNKS

_z = {}  # tag -> the model's Z[0 ... N_ROWS] of the argument, one argument_product each


@pytest.fixture(scope="module")
def run(pkg, ctx, oracle):
    """The one device run: (world, arena, z, closing, report)"""
    import torch
    assert N_SETS == 1 and min(N_ROWS, (1 << K) - 1) // 1024 + 1 == 257
    table, d_table = gp.compressed_table(oracle)
    host = gp.columns(N_SETS, gc.MANY_CHUNKS_SEED, 1 << K)
    inv, rep = ctx.invert_table(d_table, gp.BETA, gp.GAMMA)
    assert not rep["noncanonical"]
    w = dict(n_sets=N_SETS, host=host, dev=[torch.from_numpy(c.astype(np.uint32).view(np.int32)).cuda() for c in host], inv=inv, d_table=d_table,
             d_beta=gp.cell(gp.BETA), d_gamma=gp.cell(gp.GAMMA), tables=[gm.values(t) for t in table])
    arena = G.DeviceArena(G.CANARIES[1])
    z, closing, report = gp.product(pkg, ctx, arena, w, N_ROWS, PAD, k=K)
    yield w, arena, z, closing, report
    _z.clear()


def model(w, tag):
    if tag not in _z:
        cols = [c[0, tag - 1, :N_ROWS] for c in w["host"]]
        _z[tag] = gm.argument_product(w["tables"][gm.TABLE_OF_TAG[tag]], *cols, gp.BETA, gp.GAMMA, PAD)
    return _z[tag]


@pytest.mark.parametrize("tag", gm.TAGS)
def test_an_argument_of_257_chunks_is_the_models_cell_for_cell(run, tag):
    import torch
    w, _arena, z, closing, _report = run
    exp = model(w, tag)
    assert len(exp) == N_ROWS + 1 and exp[0] == 1 and all(exp)  # random columns: no zero term
    bad = torch.nonzero((z[0, tag - 1, :N_ROWS + 1] != torch.from_numpy(gm.cells(exp).copy()).cuda()).any(dim=1))
    assert not bad.numel(), "tag %d: %d cells of Z differ, first row %d" % (tag, len(bad), int(bad[0]))
    assert bytes(closing[0, tag - 1].cpu().numpy()) == bytes(gm.cells([exp[N_ROWS]])[0])


def test_the_report_the_poison_above_the_closing_row_and_the_guard_bands(pkg, run):
    import torch
    w, arena, z, closing, report = run
    zs = [[model(w, tag) for tag in gm.TAGS]]
    assert len({arg[N_ROWS] for arg in zs[0]}) == 5 and 1 not in {arg[N_ROWS] for arg in zs[0]}  # five distinct products, all open
    assert gm.report(zs, N_ROWS) == {"arguments": 5, "open": 5, "first_open": (0, 1)}
    assert pkg.api.grand_report_dict(report.view(torch.int64)) == gm.report(zs, N_ROWS)
    assert np.array_equal(closing.cpu().numpy(), gm.cells([arg[N_ROWS] for arg in zs[0]]).reshape(1, 5, 32))
    assert bytes(z[0, 0, 0].cpu().numpy()) == gm.ONE_CELL
    assert arena.poisoned_on_device(z[:, :, N_ROWS + 1:]), "a row above the closing product was written"
    arena.check_on_device()
