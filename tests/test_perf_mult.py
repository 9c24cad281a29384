"""Timing condition of the lookup multiplicities (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot
redden the parity suite).  No absolute time is fixed: the default form is compared with aesw_circ_check_witness_device in the
same process over the same 2^20-block PACKED batch of K = 20 / N = 4 circuits, alternating, median of five.  Both read the same
slab bytes once; the checker walks 1 360 rows and 1 952 copy edges per block, the count 1 360 rows with at most one add each.  A
count that loses to it is bound by its adds, not by memory.  Every figure is printed before it is asserted (run with -s)."""
import ctypes as C

import pytest

from test_perf_circ_check import _alternate, _batch, _one_launch, gpu  # noqa: F401  (the method and the fixture)

pytestmark = pytest.mark.perf


def test_the_count_beats_the_many_circuit_check(gpu, pkg):
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets = 20, 4
        nc = (1 << 20) // pkg.block_capacity(k, n_sets)
        cap, keys, pt, kw, w, offs = _batch(torch, pkg, ctx, k, n_sets, nc, 5)
        n = cap * nc
        rep8 = torch.empty(8, dtype=torch.int64, device="cuda")
        check = _one_launch(pkg, ctx, k, n_sets, nc, n, keys, pt, kw, w, offs, rep8)
        lib = pkg.api.load_mult_library()
        mult = torch.empty((nc, n_sets, pkg.TABLE_ROWS), dtype=torch.int32, device="cuda")
        rep3 = torch.empty(3, dtype=torch.int64, device="cuda")
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
        args = (ctx._h, k, n_sets, nc, offs.data_ptr(), pkg.LAYOUT_PACKED, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(), C.byref(ks),
                mult.data_ptr(), rep3.data_ptr(), ctx._stream())

        def count():
            rc = lib.aesw_mult_count_device(*args)
            assert rc == 0, rc

        t_mult, t_check = _alternate(torch, count, check)
        form = {1: "direct", 2: "private"}[lib.aesw_mult_default_form(k, n_sets, nc)]
        linear = n * sum(pkg.column_stride(pkg.LAYOUT_PACKED, i) for i in range(3))
        print("\nK=20 N=4 C=%d (%d blocks): count (%s form) %.3f ms = %.0f GB/s of slab bytes, many-circuit check %.3f ms, ratio %.3f" % (
            nc, n, form, t_mult, linear / t_mult / 1e6, t_check, t_mult / t_check))
        lookups = 400 * nc + 1056 * n
        assert rep3.cpu().tolist() == [lookups, 0, -1] and int(mult.sum(dtype=torch.int64)) == lookups
        assert rep8.cpu().tolist()[:6] == [n, nc, 0, 0, 0, 0]
        assert t_mult < t_check, (t_mult, t_check)
    finally:
        ctx.close()
