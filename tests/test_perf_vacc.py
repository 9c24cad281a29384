"""Timing condition of the VALUES accumulator (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot
redden the parity suite).  One circuit at K = 24 / N = 4 filled to its capacity, 49 342 blocks: reset + add_values + add_key
against reset + add(PACKED) + add_key of the same key and plaintexts, in the same process.  Each side is captured into a graph of
its own; after a warm-up replay of each the two are replayed in turn, 21 times, and the medians compared.  No ratio is claimed:
the VALUES walk reads 1 072 bytes per block instead of 3 024 and takes 17 row steps per lane instead of 22, so it must not be
slower.  Every figure is printed before it is asserted (run with -s); the recorded run is in profiles/vacc/README.md."""
import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import _ms, gpu  # noqa: F401  (the clock and the fixture)

pytestmark = pytest.mark.perf


def test_the_values_accumulator_is_not_slower_than_the_packed_one(gpu, pkg):
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets = 24, 4
        n = pkg.block_capacity(k, n_sets)
        assert n == 49342
        rng = np.random.default_rng(24)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        kw = ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        packed = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED)
        vals = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_VALUES)
        assert pkg.api.load_vacc_library().aesw_vacc_prepare(ctx._h) == 0
        acc_p, acc_v = ctx.multiplicity_accumulator(k, n_sets), ctx.multiplicity_accumulator(k, n_sets)

        def from_packed():
            acc_p.reset().add(0, packed).add_key(kw)

        def from_values():
            acc_v.reset().add_values(0, pt, vals, kw).add_key(kw)

        g_p, g_v = _graph(torch, from_packed), _graph(torch, from_values)
        g_p.replay(), g_v.replay()
        torch.cuda.synchronize()
        t_p, t_v = [], []
        for _ in range(REPLAYS):
            t_p.append(_ms(torch, g_p.replay))
            t_v.append(_ms(torch, g_v.replay))
        t_p, t_v = sorted(t_p)[REPLAYS // 2], sorted(t_v)[REPLAYS // 2]
        chunk = pkg.api.load_vacc_library().aesw_vacc_default_chunk(k, n_sets, 0, n)
        print("\nK=24 N=4, one circuit of %d blocks: from VALUES (%d bytes, chunk %d) %.3f ms, from PACKED (%d bytes) %.3f ms, ratio %.3f; "
              "medians of %d graph replays in turn" % (n, n * 1072, chunk, t_v, n * 3024, t_p, t_v / t_p, REPLAYS))
        lookups = 400 + 1056 * n
        assert acc_v.report() == acc_p.report() == {"lookups": lookups, "misses": 0, "first_miss": None}
        assert torch.equal(acc_v.histograms(), acc_p.histograms())
        assert t_v <= t_p, (t_v, t_p)
    finally:
        ctx.close()
