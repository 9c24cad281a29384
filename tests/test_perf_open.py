"""Timing conditions of libaesw_open.so (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot redden the
parity suite).  At K = 20 with 8 seeded coefficient columns, the protocol of tests/test_perf_grand.py: every candidate is captured
into a graph of its own and, after a warm-up replay of each, the graphs are replayed in turn, 21 times; a figure is the median of a
candidate's 21 replays.  Two conditions are held:
  * evaluating the 8 columns at one point takes no longer than lagrange_to_coeff of the same 8 columns in the same session: one
    pass of about two products a cell must not lose to a transform of two passes of ten stages each.  The yardstick is existing
    code, so there is no margin;
  * one call at 4 points is faster than four calls at 1 point (captured in one graph) by more than the spread of the 1-point
    replays (largest minus smallest, measured here, not assumed).
Recorded without a bound: evaluate at 1 and at 4 points, fold, divide, and every launch by itself -- the library built with
-DAESW_OPEN_PASSES=<mask> through build_satellite(..., extra_flags, out), whose entry points enqueue that launch only.  Every
figure is printed before it is asserted (run with -s) and written to profiles/open/README.md."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import gpu  # noqa: F401  (the fixture)
from test_perf_theta import _times

pytestmark = pytest.mark.perf
ROOT = Path(__file__).resolve().parent.parent
PASSES = {"powers": 1, "chunk": 2, "carry": 4, "scan": 8}  # AESW_OPEN_PASSES of open/aesw_open.hip; the fold is one launch as it is


def test_one_point_is_no_slower_than_a_transform_and_four_points_share_the_read(gpu, pkg):
    torch = gpu
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    api = pkg.api
    shipped = api.load_open_library()
    libs = {name: api.load_open_library(b.build_satellite("open", extra_flags=["-DAESW_OPEN_PASSES=%d" % mask], out="libaesw_open_perf_%s.so" % name))
            for name, mask in PASSES.items()}
    ctx = pkg.Context(0)
    try:
        k, n_cols = 20, 8
        rng = np.random.default_rng(20)
        cells = rng.integers(0, 256, (n_cols, 1 << k, 32), dtype=np.uint8)
        cells[:, :, 31] &= 0x1f  # canonical: below r = 0x3064...
        coeff = torch.from_numpy(cells).cuda()
        points = torch.from_numpy(np.stack([api.fr_cell(int.from_bytes(rng.bytes(40), "little")) for _ in range(4)])).cuda()
        tables = ctx.ntt_tables(k)
        transformed, quot = torch.empty_like(coeff), torch.empty_like(coeff)
        folded = torch.empty((1 << k, 32), dtype=torch.uint8, device="cuda")
        evals, rem = torch.empty((n_cols, 4, 32), dtype=torch.uint8, device="cuda"), torch.empty((n_cols, 32), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(shipped.aesw_open_workspace_bytes(k, n_cols, 4)), dtype=torch.uint8, device="cuda")

        def evaluate(lib, n_points, first=0):
            def call():
                rc = lib.aesw_open_evaluate_device(ctx._h, k, n_cols, n_points, coeff.data_ptr(), points[first:].data_ptr(), evals.data_ptr(), ws.data_ptr(), ctx._stream())
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return call

        def divide(lib):
            def call():
                rc = lib.aesw_open_divide_device(ctx._h, k, n_cols, coeff.data_ptr(), points.data_ptr(), quot.data_ptr(), rem.data_ptr(), ws.data_ptr(), ctx._stream())
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return call

        def four_calls():
            for p in range(4):
                evaluate(shipped, 1, p)()

        # what is timed computes what it should: the remainder is the evaluation, and four points are four times one point
        evaluate(shipped, 4)()
        four = evals.clone()
        divide(shipped)()
        torch.cuda.synchronize()
        assert torch.equal(rem, four[:, 0])
        for p in range(4):
            evaluate(shipped, 1, p)()
            torch.cuda.synchronize()
            assert torch.equal(evals.view(-1, 32)[:n_cols], four[:, p]), p

        names = ["eval1", "eval4", "four1", "divide", "fold", "l2c"]
        graphs = [_graph(torch, evaluate(shipped, 1)), _graph(torch, evaluate(shipped, 4)), _graph(torch, four_calls), _graph(torch, divide(shipped)),
                  _graph(torch, lambda: ctx.fold_columns(coeff, k, points[0], out=folded)), _graph(torch, lambda: ctx.lagrange_to_coeff(coeff, k, tables, out=transformed))]
        for name in PASSES:
            names += [name + "/evaluate", name + "/divide"] if name != "scan" else [name + "/divide"]
            graphs += [_graph(torch, evaluate(libs[name], 1)), _graph(torch, divide(libs[name]))] if name != "scan" else [_graph(torch, divide(libs[name]))]
        t = dict(zip(names, _times(torch, graphs)))
        m = {name: ts[REPLAYS // 2] for name, ts in t.items()}
        spread1 = t["eval1"][-1] - t["eval1"][0]
        read = n_cols * (32 << k)
        lines = [
            "# Coefficient columns at a point, measured (`tests/test_perf_open.py`, `pytest -m perf -s`)",
            "",
            "K = 20, 8 seeded coefficient columns (%d bytes).  Every figure is the median of %d graph replays taken in turn with the other" % (read, REPLAYS),
            "candidates after a warm-up replay of each, in one process on one lease.  A launch by itself is the library built with",
            "`-DAESW_OPEN_PASSES=<mask>`.",
            "",
            "| what | median |",
            "|---|---|",
            "| `evaluate_columns`, 1 point, three launches | %.3f ms |" % m["eval1"],
            "| spread of that across its %d replays (largest - smallest) | %.3f ms |" % (REPLAYS, spread1),
            "| `evaluate_columns`, 4 points in one call | %.3f ms |" % m["eval4"],
            "| four calls of `evaluate_columns` at 1 point, one graph | %.3f ms |" % m["four1"],
            "| `divide_columns`, four launches (%d bytes of quotient written) | %.3f ms |" % (read, m["divide"]),
            "| `fold_columns` of the 8 columns, one launch | %.3f ms |" % m["fold"],
            "| `lagrange_to_coeff` of the same 8 columns, out of place (the yardstick) | %.3f ms |" % m["l2c"],
            "| `open_powers_kernel` alone | %.3f ms |" % m["powers/evaluate"],
            "| `open_chunk_kernel` alone, 1 point | %.3f ms |" % m["chunk/evaluate"],
            "| `open_carry_kernel` alone, evaluate (8 workgroups, 4 turns each) | %.3f ms |" % m["carry/evaluate"],
            "| `open_carry_kernel` alone, divide (the carries written in place) | %.3f ms |" % m["carry/divide"],
            "| `open_scan_kernel<1>` alone | %.3f ms |" % m["scan/divide"],
            "",
            "Evaluating at one point reads the columns at %.2f TB/s." % (read / m["eval1"] / 1e9),
            "Condition 1: evaluate at 1 point <= lagrange_to_coeff: %.3f <= %.3f." % (m["eval1"], m["l2c"]),
            "Condition 2: four calls - one call at 4 points > spread of the 1-point replays: %.3f - %.3f > %.3f." % (m["four1"], m["eval4"], spread1),
            "",
            "**Not measured:** no `rocprofv3` trace and no counters, so nothing here says what bounds a kernel -- the field products, the",
            "128-byte-per-lane reads or the serial turns of the carry; the plain and sc1 store modes; other shapes (the",
            "carry kernel's turns grow with 2^k, its workgroups with the columns and the points); other leases.",
            "",
        ]
        print("\n" + "\n".join(lines))
        out = ROOT / "profiles" / "open" / "README.md"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines))
        assert m["eval1"] <= m["l2c"], (m["eval1"], m["l2c"])
        assert m["four1"] - m["eval4"] > spread1, (m["four1"], m["eval4"], spread1)
    finally:
        ctx.close()
