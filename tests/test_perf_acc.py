"""Timing condition of the multiplicity accumulator (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease
cannot redden the parity suite).  One circuit at K = 24 / N = 4 filled to its capacity, PACKED: reset + one add over the whole
circuit + add_key against aesw_mult_count_device over the same slabs (AUTO, which is its DIRECT form for one circuit), in the
same process.  Each side is captured into a graph of its own; after a warm-up replay of each the two are replayed in turn, 21
times, and the medians compared.  No ratio is claimed: the accumulator must not be slower.  Every figure is printed before it
is asserted (run with -s); the recorded run is in profiles/acc/README.md."""
import ctypes as C

import numpy as np
import pytest

from test_perf_circ_check import _ms, gpu  # noqa: F401  (the clock and the fixture)

pytestmark = pytest.mark.perf
REPLAYS = 21


def _graph(torch, fn):
    fn()  # once eagerly: code objects loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        fn()
    return graph


def test_the_accumulator_is_not_slower_than_the_one_shot_count(gpu, pkg):
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets, lay = 24, 4, pkg.LAYOUT_PACKED
        n = pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(24)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        kw = ctx.key_schedule_witness(key.reshape(1, 16), lay, want_rk=False)
        w = ctx.encrypt_witness(pt, key, layout=lay)
        offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, [n], n).view(np.int64)).cuda()
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
        mlib, alib = pkg.api.load_mult_library(), pkg.api.load_acc_library()
        assert mlib.aesw_mult_default_form(k, n_sets, 1) == pkg.api.MULT_FORM_DIRECT
        one = torch.empty((1, n_sets, pkg.TABLE_ROWS), dtype=torch.int32, device="cuda")
        rep_one = torch.empty(3, dtype=torch.int64, device="cuda")
        acc = ctx.multiplicity_accumulator(k, n_sets, lay)
        witness = pkg.Witness(w.x, w.y, w.z, None, None)

        def one_shot():
            rc = mlib.aesw_mult_count_device(ctx._h, k, n_sets, 1, offs.data_ptr(), lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(), C.byref(ks),
                                             one.data_ptr(), rep_one.data_ptr(), ctx._stream())
            assert rc == 0, rc

        def accumulate():
            acc.reset().add(0, witness).add_key(kw)

        g_one, g_acc = _graph(torch, one_shot), _graph(torch, accumulate)
        g_one.replay(), g_acc.replay()
        torch.cuda.synchronize()
        t_one, t_acc = [], []
        for _ in range(REPLAYS):
            t_one.append(_ms(torch, g_one.replay))
            t_acc.append(_ms(torch, g_acc.replay))
        t_one, t_acc = sorted(t_one)[REPLAYS // 2], sorted(t_acc)[REPLAYS // 2]
        chunk = alib.aesw_acc_default_chunk(k, n_sets, 0, n)
        slab_bytes = n * sum(pkg.column_stride(lay, i) for i in range(3))
        print("\nK=24 N=4, one circuit of %d blocks (%d slab bytes): accumulator (chunk %d) %.3f ms, aesw_mult_count_device (DIRECT) %.3f ms, ratio %.3f; "
              "medians of %d graph replays in turn" % (n, slab_bytes, chunk, t_acc, t_one, t_acc / t_one, REPLAYS))
        lookups = 400 + 1056 * n
        assert acc.report() == {"lookups": lookups, "misses": 0, "first_miss": None} and rep_one.cpu().tolist() == [lookups, 0, -1]
        assert torch.equal(acc.histograms(), one[0])
        assert t_acc <= t_one, (t_acc, t_one)
    finally:
        ctx.close()
