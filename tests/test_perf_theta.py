"""Timing condition of the compression under theta (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease
cannot redden the parity suite).  At K = 20 / N = 4, n_rows = 2^20, over A' of a full circuit: ONE aesw_theta_columns_device
over the 20 arguments against the TWENTY aesw_perm_gather_fr_device calls it replaces, each with the table of its argument's
arity.  Each side is captured into a graph of its own; after a warm-up replay of each the two are replayed in turn, 21 times
(the protocol of profiles/perm/README.md).  The fused call must not be slower than the twenty: median <= median + spread, where
the spread is what the baseline itself shows on this lease, the largest minus the smallest of its own 21 replays -- measured
here, not assumed.  Recorded without a bound: the compress call, and the inputs call against a fill_ of the bytes it writes.
Every figure is printed before it is asserted (run with -s) and written to profiles/theta/README.md."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import _ms, gpu  # noqa: F401  (the clock and the fixture)

pytestmark = pytest.mark.perf
ROOT = Path(__file__).resolve().parent.parent
TABLE_OF_TAG = (0, 2, 1, 1, 1)


def _times(torch, graphs):
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    ts = [[] for _ in graphs]
    for _ in range(REPLAYS):
        for t, g in zip(ts, graphs):
            t.append(_ms(torch, g.replay))
    return [sorted(t) for t in ts]


def test_the_fused_columns_call_is_not_slower_than_the_twenty_gathers(gpu, pkg):
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets, u = 20, 4, 1 << 20
        n = pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(20)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        w, kw = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED), ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        mult, rep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n])
        assert rep == {"lookups": 400 + 1056 * n, "misses": 0, "first_miss": None}
        a, _s, prep = ctx.permuted_columns(k, n_sets, mult, n_rows=u)
        assert prep["overflowed"] == 0
        theta = int.from_bytes(rng.bytes(40), "little") % pkg.api.FR_MODULUS
        d_theta = torch.from_numpy(pkg.api.fr_cell(theta)).cuda()
        table, trep = ctx.compress_table(d_theta)
        assert not trep["noncanonical"]
        out_fused = torch.empty((n_sets, 5, u, 32), dtype=torch.uint8, device="cuda")
        out_twenty = torch.empty_like(out_fused)
        tables = [table[j] for j in range(3)]

        def fused():
            ctx.argument_columns(a, table, k, n_sets, out=out_fused)

        def twenty():
            for st in range(n_sets):
                for t in range(5):
                    ctx.gather_fr(a[st, t], tables[TABLE_OF_TAG[t]], out=out_twenty[st, t])

        g_fused, g_twenty = _graph(torch, fused), _graph(torch, twenty)
        torch.cuda.synchronize()
        assert torch.equal(out_fused, out_twenty), "the fused call and the twenty gathers disagree"
        t_fused, t_twenty = _times(torch, (g_fused, g_twenty))
        m_fused, m_twenty, spread = t_fused[REPLAYS // 2], t_twenty[REPLAYS // 2], t_twenty[-1] - t_twenty[0]
        written = out_fused.numel()

        # recorded, not bounded: the compress call, and the inputs call against a fill_ of what it writes
        d_in = torch.empty((n_sets, 5, 1 << k), dtype=torch.int32, device="cuda")
        irep, crep = torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
        lib = pkg.api.load_theta_library()
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
        side = torch.cuda.Stream()
        handle = C.c_void_p(side.cuda_stream)
        assert lib.aesw_theta_prepare(ctx._h, k, n_sets, handle) == 0

        def inputs(stream=None):
            rc = lib.aesw_theta_inputs_device(ctx._h, k, n_sets, n, pkg.LAYOUT_PACKED, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(), C.byref(ks),
                                              d_in.data_ptr(), irep.data_ptr(), ctx._stream() if stream is None else stream)
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

        inputs()
        torch.cuda.synchronize()
        assert pkg.api.mult_report_dict(irep) == rep
        g_inputs = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_inputs, stream=side):
            inputs(handle)
        g_fill = _graph(torch, lambda: d_in.fill_(66560))
        g_compress = _graph(torch, lambda: lib.aesw_theta_compress_table_device(ctx._h, d_theta.data_ptr(), table.data_ptr(), crep.data_ptr(), ctx._stream()))
        t_inputs, t_fill, t_compress = [t[REPLAYS // 2] for t in _times(torch, (g_inputs, g_fill, g_compress))]
        in_bytes = d_in.numel() * 4
        lines = [
            "# The compression under theta, measured (`tests/test_perf_theta.py`, `pytest -m perf -s`)",
            "",
            "K = 20 / N = 4, a full circuit (%d blocks), `n_rows = 2^20`.  Every figure is the median of %d graph replays taken in turn" % (n, REPLAYS),
            "with the other candidates after a warm-up replay of each, in one process on one lease.",
            "",
            "| what | median |",
            "|---|---|",
            "| `argument_columns`, one call over the 20 arguments of `A'` (%d bytes written) | %.3f ms = %.2f TB/s |" % (written, m_fused, written / m_fused / 1e9),
            "| twenty `gather_fr` calls, one per argument (the same bytes) | %.3f ms = %.2f TB/s |" % (m_twenty, written / m_twenty / 1e9),
            "| spread of the twenty calls across their %d replays (largest - smallest) | %.3f ms |" % (REPLAYS, spread),
            "| `compress_table` (3 x 66 561 cells) | %.3f ms |" % t_compress,
            "| `aesw_theta_inputs_device`, both launches (%d bytes written) | %.3f ms = %.2f TB/s |" % (in_bytes, t_inputs, in_bytes / t_inputs / 1e9),
            "| `fill_` of the same bytes | %.3f ms = %.2f TB/s |" % (t_fill, in_bytes / t_fill / 1e9),
            "",
            "Criterion: fused median <= baseline median + baseline spread: %.3f <= %.3f + %.3f." % (m_fused, m_twenty, spread),
            "The inputs call runs at %.2f of the rate of a fill; it has no bound." % (t_fill / t_inputs),
            "",
            "**Not measured:** no `rocprofv3` trace and no counters, so the split of the inputs call between `theta_inputs_kernel` and",
            "`theta_report_kernel` is not known; `n_rows < 2^k`; the plain and sc1 store modes; DENSE slabs; other shapes; other leases.",
            "",
        ]
        print("\n" + "\n".join(lines))
        out = ROOT / "profiles" / "theta" / "README.md"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines))
        assert m_fused <= m_twenty + spread, (m_fused, m_twenty, spread)
    finally:
        ctx.close()
