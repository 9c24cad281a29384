"""libaesw_quot.so on the GPU: sigma as cells against sigma_model.label, every cell, below and above the 14-bit split of the
permutation's power tables (qc.SIGMA_FR), into poisoned, guard-banded outputs -- every cell written, every guard intact, an entry
out of range read as the cell itself -- and every refusal, which leaves the output alone."""
import numpy as np
import pytest

import guarded
import ntt_model as nm
import quot_cases as qc
import sigma_model as sm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,n_cols", qc.SIGMA_FR)
def test_sigma_as_cells_is_the_label_of_every_entry(ctx, k, n_cols):
    import torch
    n = 1 << k
    rng = np.random.default_rng(0x7367 + k)
    mapping = rng.integers(0, n_cols * n, (n_cols, n), dtype=np.int64).astype(np.uint32)
    mapping[0, 0], mapping[n_cols - 1, n - 1], mapping[1, 5] = n_cols * n - 1, 0, 0xFFFFFFFF  # the last cell; the first; out of range: the cell itself
    mapping[2, 7] = n_cols * n
    sigma_tables = ctx.permutation_tables(k, n_cols)
    arena = guarded.DeviceArena(guarded.CANARIES[k % 2])
    out = arena.out("sigma_fr", n_cols * n * 32, (n_cols, n, 32))
    ctx.permutation_columns_fr(k, n_cols, mapping, sigma_tables, _out=out)
    torch.cuda.synchronize()
    arena.check()
    w, acc, w_pows = sm.omega(k), 1, []
    for _ in range(n):
        w_pows.append(acc)
        acc = acc * w % sm.R
    d_pows = [pow(sm.DELTA, c, sm.R) for c in range(n_cols)]
    image = np.where(mapping.astype(np.int64) >= n_cols * n, np.arange(n_cols * n).reshape(n_cols, n), mapping.astype(np.int64))
    exp = nm.to_cells([sm.label(k, w_pows, d_pows, int(m)) for m in image.reshape(-1)])
    guarded.assert_bytes("sigma_fr", out.cpu().numpy().reshape(-1, 32), exp)
    assert image[1, 5] == n + 5 and image[2, 7] == 2 * n + 7


def test_every_bound_and_an_overlapping_output_are_refused(pkg, ctx):
    import torch
    lib = pkg.api.load_quot_library()
    bad, poison = pkg.api.ERR_INVALID_ARG, 0xA5
    sigma_tables = ctx.permutation_tables(10, 5)
    mapping = torch.zeros((5, 1024), dtype=torch.int32, device="cuda")
    sigma = torch.full((5, 1024, 32), poison, dtype=torch.uint8, device="cuda")
    for kk, n_cols, map_ptr, tables_ptr, out_ptr in ((9, 5, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (29, 5, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (10, 0, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (10, 3075, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (10, 5, 0, sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (10, 5, mapping.data_ptr(), 0, sigma.data_ptr()),
                                                     (10, 5, mapping.data_ptr(), sigma_tables.data_ptr(), 0),
                                                     (10, 5, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr() + 4),
                                                     (10, 5, sigma.data_ptr() + 64, sigma_tables.data_ptr(), sigma.data_ptr()),
                                                     (10, 5, mapping.data_ptr(), sigma.data_ptr() + 5 * 1024 * 32 - 32, sigma.data_ptr())):
        assert lib.aesw_quot_sigma_fr_device(ctx._h, kk, n_cols, map_ptr, tables_ptr, out_ptr, ctx._stream()) == bad, (kk, n_cols)
    torch.cuda.synchronize()
    assert bool((sigma == poison).all()), "a refused call wrote"
    with pytest.raises(pkg.AeswError):
        ctx.permutation_columns_fr(9, 5, mapping, sigma_tables)
    with pytest.raises(ValueError):
        ctx.permutation_columns_fr(10, 5, mapping[:4], sigma_tables)
    assert lib.aesw_quot_sigma_fr_device(ctx._h, 10, 5, mapping.data_ptr(), sigma_tables.data_ptr(), sigma.data_ptr(), ctx._stream()) == 0  # the call they were cut from
    torch.cuda.synchronize()
    assert not bool((sigma == poison).all())
