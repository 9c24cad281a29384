"""Timing of the permutation argument's grand products (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease
cannot redden the parity suite).  At K = 20 / N = 4 over a full circuit -- 14 columns, chunk_len 3, 5 sets, n_rows = 2^20 - 6 -- the
protocol of tests/test_perf_grand.py: every candidate is captured into a graph of its own and, after a warm-up replay of each, the
graphs are replayed in turn, 21 times; a figure is the median of a candidate's 21 replays.  Recorded: permutation_product as a
whole and launch by launch (the library built with -DAESW_SIGMA_PASSES=<mask>, whose entry point enqueues those launches only),
the tables call, and grand_product over the same circuit from the same session.  One condition is held:
  * the product's time per Z cell written is at most (chunk_len + 1) times grand_product's time per Z cell, plus the spread of
    grand_product's own replays (largest minus smallest, per cell).  The margin is an estimate from instruction counts -- about
    10 * chunk_len + 2 field products per row over both passes against ten -- and was not measured before it was set.
Every figure is printed before it is asserted (run with -s) and written to profiles/sigma/README.md.

The recorded run does NOT hold the condition: permutation_product 5.023 ms for 5 242 855 cells (0.9581 ns per cell), grand_product
2.999 ms for 20 971 420 cells (0.1430 ns per cell, spread 0.0037 ns): 6.70 times, against a bound of 0.5758 ns.  Nothing was changed
to make it hold ("Measured")."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import gpu  # noqa: F401  (the fixture)
from test_perf_theta import _times

pytestmark = pytest.mark.perf
ROOT = Path(__file__).resolve().parent.parent
PASSES = {"prepare": 1, "chunk": 2, "carry": 4, "chain": 8, "scan": 16}  # AESW_SIGMA_PASSES of sigma/aesw_sigma.hip


def test_the_product_per_cell_stays_within_chunk_len_plus_one_lookup_products(gpu, pkg):
    torch = gpu
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    api = pkg.api
    shipped = api.load_sigma_library()
    libs = {name: api.load_sigma_library(b.build_satellite("sigma", extra_flags=["-DAESW_SIGMA_PASSES=%d" % mask], out="libaesw_sigma_perf_%s.so" % name))
            for name, mask in PASSES.items()}
    ctx = pkg.Context(0)
    try:
        k, n_sets, chunk_len, u = 20, 4, 3, (1 << 20) - 6
        n = pkg.block_capacity(k, n_sets)
        n_cols = api.permutation_columns(n_sets)
        sets = -(-n_cols // chunk_len)
        assert (n_cols, sets) == (14, 5) and api.block_placement(k, n_sets, n - 1)[1] + pkg.AES_ROWS <= u
        rng = np.random.default_rng(20)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        w, kw = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED), ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        theta, beta, gamma = (int.from_bytes(rng.bytes(40), "little") % api.FR_MODULUS for _ in range(3))
        d_theta, d_beta, d_gamma = (torch.from_numpy(api.fr_cell(v)).cuda() for v in (theta, beta, gamma))
        # the permutation argument
        advice = ctx.assemble_advice(k, n_sets, w, kw, n, layout=pkg.LAYOUT_PACKED)
        fixed = np.zeros((1, 1 << k), np.uint8)
        fixed[0, :96] = pkg.selector_tags()[3]
        fixed = torch.from_numpy(fixed).cuda()
        source = torch.from_numpy(api.permutation_sources(n_sets).view(np.int32)).cuda()
        mapping = torch.from_numpy(api.permutation_mapping(k, n_sets, n).view(np.int32)).cuda()
        tables = ctx.permutation_tables(k, n_cols)
        z = torch.empty((sets, 1 << k, 32), dtype=torch.uint8, device="cuda")
        closing = torch.empty((sets, 32), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(shipped.aesw_sigma_workspace_bytes(k, n_cols, chunk_len)), dtype=torch.uint8, device="cuda")
        _z, _c, rep = ctx.permutation_product(k, n_cols, chunk_len, advice, fixed, source, mapping, tables, d_beta, d_gamma, n_rows=u, _out=(z, closing), _workspace=ws)
        assert rep == {"sets": 5, "open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}
        scratch_rep = torch.empty(6, dtype=torch.int64, device="cuda")

        def product(lib):
            def call():
                rc = lib.aesw_sigma_product_device(ctx._h, k, n_cols, chunk_len, u, advice.data_ptr(), 3 * n_sets + 1, fixed.data_ptr(), 1, source.data_ptr(),
                                                   mapping.data_ptr(), tables.data_ptr(), d_beta.data_ptr(), d_gamma.data_ptr(), z.data_ptr(), closing.data_ptr(),
                                                   ws.data_ptr(), scratch_rep.data_ptr(), ctx._stream())
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return call
        # the lookup grand product over the same circuit
        mult, mrep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n])
        assert mrep["misses"] == 0
        a, s, _prep = ctx.permuted_columns(k, n_sets, mult, n_rows=u)
        inputs, _ = ctx.lookup_inputs(k, n_sets, w, kw)
        table, _trep = ctx.compress_table(d_theta)
        inv, _vrep = ctx.invert_table(table, d_beta, d_gamma)
        grand = api.load_grand_library()
        gz = torch.empty((n_sets, 5, 1 << k, 32), dtype=torch.uint8, device="cuda")
        gclosing = torch.empty((n_sets, 5, 32), dtype=torch.uint8, device="cuda")
        gws = torch.empty(int(grand.aesw_grand_workspace_bytes(k, n_sets)), dtype=torch.uint8, device="cuda")
        _gz, _gc, grep = ctx.grand_product(k, n_sets, inputs, a, s, table, inv, d_beta, d_gamma, n_rows=u, _out=(gz, gclosing), _workspace=gws)
        assert grep == {"arguments": 20, "open": 0, "first_open": None}

        def grand_call():
            rc = grand.aesw_grand_product_device(ctx._h, k, n_sets, u, 0, inputs.data_ptr(), a.data_ptr(), s.data_ptr(), table.data_ptr(), inv.data_ptr(),
                                                 d_beta.data_ptr(), d_gamma.data_ptr(), gz.data_ptr(), gclosing.data_ptr(), gws.data_ptr(), scratch_rep.data_ptr(), ctx._stream())
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

        names = ["product"] + list(PASSES) + ["grand", "tables"]
        graphs = [_graph(torch, product(shipped))] + [_graph(torch, product(libs[name])) for name in PASSES] + \
            [_graph(torch, grand_call), _graph(torch, lambda: ctx.permutation_tables(k, n_cols, _out=tables))]
        t = dict(zip(names, _times(torch, graphs)))
        m = {name: ts[REPLAYS // 2] for name, ts in t.items()}
        cells, gcells = sets * (u + 1), n_sets * 5 * (u + 1)
        per, gper = m["product"] * 1e6 / cells, m["grand"] * 1e6 / gcells  # ns per Z cell
        gspread = (t["grand"][-1] - t["grand"][0]) * 1e6 / gcells
        bound = (chunk_len + 1) * gper + gspread
        lines = [
            "# The permutation argument's grand products, measured (`tests/test_perf_sigma.py`, `pytest -m perf -s`)",
            "",
            "K = 20 / N = 4, a full circuit (%d blocks): 14 columns, chunk_len 3, 5 sets, `n_rows = 2^20 - 6`.  Every figure is the median of %d" % (n, REPLAYS),
            "graph replays taken in turn with the other candidates after a warm-up replay of each, in one process on one lease.  A launch",
            "by itself is the library built with `-DAESW_SIGMA_PASSES=<mask>`.",
            "",
            "| what | median |",
            "|---|---|",
            "| `permutation_product`, all five launches (%d cells of Z written) | %.3f ms |" % (cells, m["product"]),
            "| `sigma_prepare_kernel` alone (beta * delta^c, 14 cells) | %.3f ms |" % m["prepare"],
            "| `sigma_chunk_kernel` alone | %.3f ms |" % m["chunk"],
            "| `sigma_carry_kernel` alone (5 workgroups, 4 turns each way, one `fr_inv` each) | %.3f ms |" % m["carry"],
            "| `sigma_chain_kernel` alone (one workgroup) | %.3f ms |" % m["chain"],
            "| `sigma_scan_kernel<1>` alone | %.3f ms |" % m["scan"],
            "| `permutation_tables` (2^14 + 2^6 + 14 cells) | %.3f ms |" % m["tables"],
            "| `grand_product` over the same circuit (20 arguments, %d cells of Z written) | %.3f ms |" % (gcells, m["grand"]),
            "| spread of `grand_product` across its %d replays (largest - smallest) | %.3f ms |" % (REPLAYS, t["grand"][-1] - t["grand"][0]),
            "",
            "Per Z cell written: `permutation_product` %.4f ns, `grand_product` %.4f ns (spread %.4f ns): %.2f times." % (per, gper, gspread, per / gper),
            "Criterion: product per cell <= (chunk_len + 1) x grand_product per cell + its spread: %.4f <= %.4f: %s." % (per, bound, "held" if per <= bound else "NOT held"),
            "",
            "Only the suffix form (one `fr_inv` per set, two scans) was built; a lane-batched inversion in the manner of 4.20 was not, so there",
            "is no second figure to set against it.",
            "",
            "**Not measured:** no `rocprofv3` trace and no counters, so nothing here says what bounds a kernel -- the field products, the",
            "gathers of the power tables, the instruction fetch of the long straight-line code or the one wave per SIMD that the chunk and",
            "scan kernels' registers allow; two rows per lane; the plain and sc1 store modes; other shapes and chunk lengths; other leases.",
            "",
        ]
        print("\n" + "\n".join(lines))
        out = ROOT / "profiles" / "sigma" / "README.md"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines))
        assert per <= bound, (per, gper, gspread, bound)
    finally:
        ctx.close()
