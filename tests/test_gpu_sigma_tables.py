"""aesw_sigma_tables_device / Context.permutation_tables on the GPU: every cell of the three power tables against pow, for k
below, at and above the split of omega's exponent (tests/sigma_cases.py: sc.TABLE_KS x sc.TABLE_COLS), on a poisoned, guard-banded
output; the refusals leave it untouched."""
import numpy as np
import pytest

import guarded as G
import sigma_cases as sc
import sigma_model as sm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_cols", sc.TABLE_COLS)
@pytest.mark.parametrize("k", sc.TABLE_KS)
def test_every_cell_is_the_power_it_stands_for(pkg, ctx, k, n_cols):
    lib = pkg.api.load_sigma_library()
    exp = sm.tables(k, n_cols)
    need = int(lib.aesw_sigma_tables_bytes(k, n_cols))
    assert need == 32 * len(exp) == 32 * ((1 << min(k, 14)) + (1 << max(k - 14, 0)) + n_cols)
    arena = G.DeviceArena(G.CANARIES[(k + n_cols) % 2])
    out = arena.out("tables", need, (len(exp), 32))
    got = ctx.permutation_tables(k, n_cols, _out=out)
    arena.check()
    cells = got.cpu().numpy()
    exp_cells = sm.cells(exp)
    bad = np.argwhere((cells != exp_cells).any(axis=1))
    assert not bad.size, "%d cells differ, first %d" % (len(bad), bad[0][0])
    low = 1 << min(k, 14)
    w = sm.omega(k)
    for i in (0, 1, (1 << k) - 1, (1 << k) // 2 + 3, 12345 % (1 << k)):  # omega^i is one product of two cells
        assert exp[i & 16383] * exp[low + (i >> 14)] % sm.R == pow(w, i, sm.R)


def test_the_refusals_leave_the_output_untouched(pkg, ctx):
    lib = pkg.api.load_sigma_library()
    arena = G.DeviceArena()
    out = arena.out("tables", int(lib.aesw_sigma_tables_bytes(10, 3)))
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    for k, n_cols, ptr, word in ((9, 3, out.data_ptr(), "k must be"), (29, 3, out.data_ptr(), "k must be"), (10, 0, out.data_ptr(), "n_cols"),
                                 (10, 3075, out.data_ptr(), "n_cols"), (28, 17, out.data_ptr(), "2^32"), (10, 3, None, "d_tables"),
                                 (10, 3, out.data_ptr() + 4, "d_tables")):
        assert lib.aesw_sigma_tables_device(ctx._h, k, n_cols, ptr, ctx._stream()) == 1, (k, n_cols)
        assert "aesw_sigma_tables_device" in err() and word in err(), err()
        assert int(lib.aesw_sigma_tables_bytes(k, n_cols)) == (0 if ptr == out.data_ptr() else 32 * (1024 + 1 + 3))
    arena.check()
    assert arena.poisoned(out)
    group = pkg.Group([0])
    try:
        assert lib.aesw_sigma_tables_device(group._h, 10, 3, out.data_ptr(), ctx._stream()) == 1
        with pytest.raises(pkg.AeswError):
            group.permutation_tables(10, 3)
    finally:
        group.close()
    assert arena.poisoned(out)
