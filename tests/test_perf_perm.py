"""Timing condition of the permuted columns (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot
redden the parity suite).  "Counting instead of sorting" is the claim, so the yardstick is the sort: at K = 20 / N = 4, over the
histograms of a full circuit from the accumulator, aesw_perm_build_device for all 20 arguments against torch.sort over the same
twenty 2^20-element input-index columns (A' shuffled) on the same device.  Each side is captured into a graph of its own; after
a warm-up replay of each the two are replayed in turn, 21 times, and the medians compared.  The build must not be slower than
the sort alone -- which does half the job: it builds no S'.  Recorded without a bound: the build against a fill_ of the bytes it
writes, and gather_fr against expand_fr over as many cells.  Every figure is printed before it is asserted (run with -s); the
recorded run is in profiles/perm/README.md."""
import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import _ms, gpu  # noqa: F401  (the clock and the fixture)

pytestmark = pytest.mark.perf


def _medians(torch, graphs):
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    ts = [[] for _ in graphs]
    for _ in range(REPLAYS):
        for t, g in zip(ts, graphs):
            t.append(_ms(torch, g.replay))
    return [sorted(t)[REPLAYS // 2] for t in ts]


def test_the_build_is_not_slower_than_the_sort_it_replaces(gpu, pkg):
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets, u = 20, 4, 1 << 20
        n = pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(20)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        acc = ctx.multiplicity_accumulator(k, n_sets).reset()
        acc.add(0, ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED)).add_key(ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False))
        assert acc.report() == {"lookups": 400 + 1056 * n, "misses": 0, "first_miss": None}
        mult = acc.histograms()
        lib = pkg.api.load_perm_library()
        shape = (n_sets, 5, 1 << k)
        a, s = torch.empty(shape, dtype=torch.int32, device="cuda"), torch.empty(shape, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.aesw_perm_workspace_bytes(n_sets)), dtype=torch.uint8, device="cuda")
        rep = torch.empty(3, dtype=torch.int64, device="cuda")

        def build():
            rc = lib.aesw_perm_build_device(ctx._h, k, n_sets, u, 0, mult.data_ptr(), a.data_ptr(), s.data_ptr(), ws.data_ptr(), rep.data_ptr(), ctx._stream())
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

        build()
        torch.cuda.synchronize()
        assert pkg.api.perm_report_dict(rep) == {"arguments": 20, "overflowed": 0, "first_overflow": None}
        # the columns a sorting prover starts from: every argument's inputs in some row order
        inputs = torch.stack([col[torch.randperm(u, device="cuda")] for col in a.view(20, u)]).contiguous()
        sorted_out, order_out = torch.empty_like(inputs), torch.empty(inputs.shape, dtype=torch.int64, device="cuda")

        def sort():
            torch.sort(inputs, dim=1, out=(sorted_out, order_out))

        def fill():
            a.fill_(1), s.fill_(2)

        g_build, g_sort = _graph(torch, build), _graph(torch, sort)
        torch.cuda.synchronize()
        assert torch.equal(sorted_out, a.view(20, u)), "the sort and the count disagree on A'"
        g_fill = _graph(torch, fill)  # overwrites a and s: after the comparison
        t_build, t_sort, t_fill = _medians(torch, (g_build, g_sort, g_fill))
        written = 2 * 20 * u * 4
        print("\nK=20 N=4, %d blocks, 20 arguments of 2^20 rows: build (A' and S', %d bytes) %.3f ms = %.2f TB/s, torch.sort of the 20 input "
              "columns (A' alone) %.3f ms, ratio %.3f; fill_ of the same bytes %.3f ms = %.2f TB/s; medians of %d graph replays in turn"
              % (n, written, t_build, written / t_build / 1e9, t_sort, t_build / t_sort, t_fill, written / t_fill / 1e9, REPLAYS))

        # the gather against expand_fr over as many cells
        cells = 20 * u
        table = torch.from_numpy(rng.integers(0, 256, (66561, 32), dtype=np.uint8)).cuda()
        bytes_in = torch.from_numpy(rng.integers(0, 256, cells, dtype=np.uint8)).cuda()
        g_build.replay()  # a holds the columns again (fill_ ran last)
        out = torch.empty((cells, 32), dtype=torch.uint8, device="cuda")
        g_gather = _graph(torch, lambda: ctx.gather_fr(a.view(-1), table, out=out))
        g_expand = _graph(torch, lambda: ctx.expand_fr(bytes_in, out=out))
        t_gather, t_expand = _medians(torch, (g_gather, g_expand))
        print("gather_fr of %d cells %.3f ms = %.2f TB/s written, expand_fr of as many %.3f ms = %.2f TB/s"
              % (cells, t_gather, cells * 32 / t_gather / 1e9, t_expand, cells * 32 / t_expand / 1e9))
        assert t_build <= t_sort, (t_build, t_sort)
    finally:
        ctx.close()
