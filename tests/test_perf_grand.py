"""Timing conditions of the lookup grand product (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot
redden the parity suite).  At K = 20 / N = 4 over a full circuit, n_rows = 2^20 - 6, the protocol of tests/test_perf_theta.py:
every candidate is captured into a graph of its own and, after a warm-up replay of each, the graphs are replayed in turn, 21
times; a figure is the median of a candidate's 21 replays.  Two conditions are held:
  * the batch inversion as shipped (B rows a lane, one fr_inv) beats the lane-per-row inversion -- the same library built with
    -DAESW_GRAND_BATCH=1 through build_satellite(..., extra_flags, out) -- by more than the spread of B = 1's own replays (largest
    minus smallest, measured here, not assumed);
  * the chunk kernel alone takes no longer than the scan kernel alone: it does the same factors and no scan and no store of Z.
    One kernel is priced by a variant built with -DAESW_GRAND_PASSES=<mask>, whose entry points enqueue that launch only.
Recorded without a bound: grand_product next to argument_columns over the same 20 arguments (the same bytes written: how far
the product sits above its store floor), invert_table next to compress_table, the other B values, two rows per lane, and every
launch of the two calls by itself.  Every figure is printed before it is asserted (run with -s) and written to
profiles/grand/README.md."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import gpu  # noqa: F401  (the fixture)
from test_perf_theta import _times

pytestmark = pytest.mark.perf
ROOT = Path(__file__).resolve().parent.parent
BATCHES = (1, 4, 8, 16)  # B of the batch inversion: the values tried
PASSES = {"invert": 1, "invert_report": 2, "chunk": 4, "carry": 8, "scan": 16}  # AESW_GRAND_PASSES of grand/aesw_grand.hip


def _variant(b, tag, *flags):
    return b.build_satellite("grand", extra_flags=list(flags), out="libaesw_grand_perf_%s.so" % tag)


def test_the_batch_inversion_beats_a_lane_per_row_and_the_chunk_kernel_is_no_slower_than_the_scan(gpu, pkg):
    torch = gpu
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    api = pkg.api
    shipped = api.load_grand_library()
    kept = next(int(line.split()[2]) for line in (ROOT / "halo2-aes_amd" / "csrc" / "aesw_grand.h").read_text().splitlines()
                if line.startswith("#define AESW_GRAND_BATCH "))
    assert kept in BATCHES and kept != 1
    libs = {"B%d" % n: shipped if n == kept else api.load_grand_library(_variant(b, "b%d" % n, "-DAESW_GRAND_BATCH=%d" % n)) for n in BATCHES}
    libs["rows2"] = api.load_grand_library(_variant(b, "r2", "-DAESW_GRAND_ROWS_PER_LANE=2"))
    for name, mask in PASSES.items():
        libs[name] = api.load_grand_library(_variant(b, name, "-DAESW_GRAND_PASSES=%d" % mask))
    ctx = pkg.Context(0)
    try:
        k, n_sets, u = 20, 4, (1 << 20) - 6
        n = pkg.block_capacity(k, n_sets)
        assert api.block_placement(k, n_sets, n - 1)[1] + pkg.AES_ROWS <= u  # every block row is a usable row: the arguments close
        rng = np.random.default_rng(20)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        w, kw = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED), ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        mult, rep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n])
        assert rep["misses"] == 0
        a, s, prep = ctx.permuted_columns(k, n_sets, mult, n_rows=u)
        assert prep["overflowed"] == 0
        inputs, _ = ctx.lookup_inputs(k, n_sets, w, kw)
        theta, beta, gamma = (int.from_bytes(rng.bytes(40), "little") % api.FR_MODULUS for _ in range(3))
        d_theta, d_beta, d_gamma = (torch.from_numpy(api.fr_cell(v)).cuda() for v in (theta, beta, gamma))
        table, trep = ctx.compress_table(d_theta)
        assert not trep["noncanonical"]
        inv, vrep = ctx.invert_table(table, d_beta, d_gamma)
        assert vrep == {"cells": 6 * pkg.TABLE_ROWS, "noncanonical": False, "zero_terms": 0}
        z = torch.empty((n_sets, 5, 1 << k, 32), dtype=torch.uint8, device="cuda")
        closing = torch.empty((n_sets, 5, 32), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(shipped.aesw_grand_workspace_bytes(k, n_sets)), dtype=torch.uint8, device="cuda")
        _z, _c, grep = ctx.grand_product(k, n_sets, inputs, a, s, table, inv, d_beta, d_gamma, n_rows=u, _out=(z, closing), _workspace=ws)
        assert grep == {"arguments": 20, "open": 0, "first_open": None}
        z_shipped = z.clone()
        scratch_inv, scratch_rep = torch.empty_like(inv), torch.empty(3, dtype=torch.int64, device="cuda")
        crep = torch.empty(2, dtype=torch.int64, device="cuda")
        columns = torch.empty_like(z)

        def invert(lib):
            def call():
                rc = lib.aesw_grand_invert_table_device(ctx._h, table.data_ptr(), d_beta.data_ptr(), d_gamma.data_ptr(), scratch_inv.data_ptr(), scratch_rep.data_ptr(),
                                                        ctx._stream())
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return call

        def product(lib):
            def call():
                rc = lib.aesw_grand_product_device(ctx._h, k, n_sets, u, 0, inputs.data_ptr(), a.data_ptr(), s.data_ptr(), table.data_ptr(), inv.data_ptr(),
                                                   d_beta.data_ptr(), d_gamma.data_ptr(), z.data_ptr(), closing.data_ptr(), ws.data_ptr(), scratch_rep.data_ptr(), ctx._stream())
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return call

        # every variant that enqueues the whole call computes what the shipped library does
        for name in ["B%d" % n for n in BATCHES]:
            invert(libs[name])()
            torch.cuda.synchronize()
            assert torch.equal(scratch_inv, inv), name
        z.zero_()
        product(libs["rows2"])()
        torch.cuda.synchronize()
        assert torch.equal(z[:, :, :u + 1], z_shipped[:, :, :u + 1]), "two rows per lane"

        names = ["B%d" % n for n in BATCHES] + ["invert", "invert_report"]
        t = dict(zip(names, _times(torch, [_graph(torch, invert(libs[name])) for name in names])))
        t["compress"] = _times(torch, [_graph(torch, lambda: ctx._check(api.load_theta_library().aesw_theta_compress_table_device(
            ctx._h, d_theta.data_ptr(), table.data_ptr(), crep.data_ptr(), ctx._stream()), "compress"))])[0]
        pnames = ["product", "rows2", "chunk", "carry", "scan"]
        graphs = [_graph(torch, product(shipped if name == "product" else libs[name])) for name in pnames]
        graphs.append(_graph(torch, lambda: ctx.argument_columns(a, table, k, n_sets, n_rows=u, out=columns)))
        t.update(zip(pnames + ["columns"], _times(torch, graphs)))
        m = {name: ts[REPLAYS // 2] for name, ts in t.items()}
        spread_b1 = t["B1"][-1] - t["B1"][0]
        written = n_sets * 5 * (u + 1) * 32
        lines = [
            "# The lookup grand product, measured (`tests/test_perf_grand.py`, `pytest -m perf -s`)",
            "",
            "K = 20 / N = 4, a full circuit (%d blocks), `n_rows = 2^20 - 6`.  Every figure is the median of %d graph replays taken in turn" % (n, REPLAYS),
            "with the other candidates after a warm-up replay of each, in one process on one lease.  A launch by itself is the library",
            "built with `-DAESW_GRAND_PASSES=<mask>`, another B or rows per lane the library built with the matching `-D`.",
            "",
            "| what | median |",
            "|---|---|",
            "| `grand_product`, all four launches, 4 rows per lane (kept; %d bytes of Z written) | %.3f ms |" % (written, m["product"]),
            "| `grand_product`, all four launches, 2 rows per lane | %.3f ms |" % m["rows2"],
            "| `grand_chunk_kernel` alone | %.3f ms |" % m["chunk"],
            "| `grand_carry_kernel` alone (20 workgroups, 4 turns each) | %.3f ms |" % m["carry"],
            "| `grand_scan_kernel<1>` alone | %.3f ms |" % m["scan"],
            "| `argument_columns` over the same 20 arguments (the same rows written, less one per argument) | %.3f ms |" % m["columns"],
            "| `invert_table`, both launches, B = 1 (a lane per row) | %.3f ms |" % m["B1"],
            "| spread of B = 1 across its %d replays (largest - smallest) | %.3f ms |" % (REPLAYS, spread_b1),
        ] + ["| `invert_table`, both launches, B = %d%s | %.3f ms |" % (nb, " (kept)" if nb == kept else "", m["B%d" % nb]) for nb in BATCHES[1:]] + [
            "| `grand_invert_kernel` alone, B = %d | %.3f ms |" % (kept, m["invert"]),
            "| `grand_invert_report_kernel` alone (one workgroup over the three tables; the same for every B) | %.3f ms |" % m["invert_report"],
            "| `compress_table` (3 x 66 561 cells) | %.3f ms |" % m["compress"],
            "",
            "The product takes %.1f times what `argument_columns` takes to write the same bytes." % (m["product"] / m["columns"]),
            "Criterion 1: B = 1 median - kept median > spread of B = 1: %.3f - %.3f > %.3f." % (m["B1"], m["B%d" % kept], spread_b1),
            "Criterion 2: chunk kernel <= scan kernel: %.3f <= %.3f." % (m["chunk"], m["scan"]),
            "",
            "**Not measured:** no `rocprofv3` trace and no counters, so nothing here says what bounds a kernel -- the field products, the",
            "gathers or the instruction fetch of the long straight-line code; eight rows per lane; the plain and sc1 store modes; other",
            "shapes (the carry kernel's turns grow with 2^k); other leases.",
            "",
        ]
        print("\n" + "\n".join(lines))
        out = ROOT / "profiles" / "grand" / "README.md"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines))
        assert m["B1"] - m["B%d" % kept] > spread_b1, (m["B1"], m["B%d" % kept], spread_b1)
        assert m["chunk"] <= m["scan"], (m["chunk"], m["scan"])
    finally:
        ctx.close()
