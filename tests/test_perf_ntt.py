"""Timing of the transforms of libaesw_ntt.so (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot redden
the parity suite).  K = 20, ext_k = 22, 1 and 8 columns, the protocol of tests/test_perf_sigma.py: every candidate is captured
into a graph of its own and, after a warm-up replay of each, the graphs are replayed in turn, 21 times; a figure is the median of
a candidate's 21 replays.  Recorded: each of the four transforms over 1 and over 8 columns; 8 calls of one column each; each pass
by itself (the library built with -DAESW_NTT_PASSES=<mask>, whose entry points enqueue those passes only); lagrange_to_coeff of
a library built with -DAESW_NTT_PASS_LOG=1, one stage per pass -- the plain global-memory radix-2 -- with tables of its own; the
tables call; argument_columns as the store floor per cell and grand_product's field products per second from the same session,
both without a bound.  Two conditions are held, both against this commit's own alternative builds measured in the same session:
  * lagrange_to_coeff over 8 columns of the kept NTT_PASS_LOG beats the -DAESW_NTT_PASS_LOG=1 build by more than the spread of
    that build's replays (largest minus smallest);
  * for each of the four transforms, one call over 8 columns takes no longer than 8 calls of one column plus the spread of those
    eight calls' replays.
Every figure is printed before it is asserted (run with -s) and written to profiles/ntt/README.md."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from test_perf_acc import REPLAYS, _graph
from test_perf_circ_check import gpu  # noqa: F401  (the fixture)
from test_perf_theta import _times

pytestmark = pytest.mark.perf
ROOT = Path(__file__).resolve().parent.parent
K, EXT_K, COLS = 20, 22, 8
MASKS = {"pass 0": 1, "pass 1": 2, "pass 2": 4}  # AESW_NTT_PASSES of ntt/aesw_ntt.hip
NAMES = ("lagrange_to_coeff", "coeff_to_lagrange", "coeff_to_extended", "extended_to_coeff")


def butterflies(k, n_cols):
    return n_cols * k << (k - 1)


def test_the_lds_passes_beat_one_stage_per_pass_and_eight_columns_beat_eight_calls(gpu, pkg):
    torch = gpu
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    api = pkg.api
    shipped = api.load_ntt_library()
    masked = {name: api.load_ntt_library(b.build_satellite("ntt", extra_flags=["-DAESW_NTT_PASSES=%d" % mask], out="libaesw_ntt_perf_mask%d.so" % mask))
              for name, mask in MASKS.items()}
    plain = api.load_ntt_library(b.build_satellite("ntt", extra_flags=["-DAESW_NTT_PASS_LOG=1"], out="libaesw_ntt_perf_log1.so"))
    ctx = pkg.Context(0)
    try:
        rng = np.random.default_rng(22)
        rows, ext_rows = 1 << K, 1 << EXT_K
        col = torch.from_numpy(rng.integers(0, 256, (COLS, rows, 32), dtype=np.uint8)).cuda()
        col[:, :, 31] &= 0x1F  # canonical cells
        out = torch.empty_like(col)
        ext_in = torch.from_numpy(rng.integers(0, 256, (COLS, ext_rows, 32), dtype=np.uint8)).cuda()
        ext_in[:, :, 31] &= 0x1F
        ext_out = torch.empty_like(ext_in)
        tables = ctx.ntt_tables(EXT_K)
        tables_plain = torch.empty(int(plain.aesw_ntt_tables_bytes(EXT_K)), dtype=torch.uint8, device="cuda")
        assert plain.aesw_ntt_tables_device(ctx._h, EXT_K, tables_plain.data_ptr(), ctx._stream()) == 0

        def call(lib, name, n_cols, first=0, tab=tables):
            """`name` over columns first ... first + n_cols - 1, out of place"""
            def go():
                s = ctx._stream()
                if name == "coeff_to_extended":
                    rc = lib.aesw_ntt_coeff_to_extended_device(ctx._h, K, EXT_K, 1, n_cols, col[first].data_ptr(), ext_out[first].data_ptr(), tab.data_ptr(), EXT_K, None, s)
                elif name == "extended_to_coeff":
                    rc = lib.aesw_ntt_extended_to_coeff_device(ctx._h, EXT_K, 1, n_cols, ext_in[first].data_ptr(), ext_out[first].data_ptr(), tab.data_ptr(), EXT_K, None, s)
                else:
                    rc = getattr(lib, "aesw_ntt_%s_device" % name)(ctx._h, K, n_cols, col[first].data_ptr(), out[first].data_ptr(), tab.data_ptr(), EXT_K, None, s)
                assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
            return go

        def eight(name):
            calls = [call(shipped, name, 1, c) for c in range(COLS)]
            return lambda: [f() for f in calls]

        # the two builds agree before either is timed
        call(shipped, "lagrange_to_coeff", COLS)()
        kept = out.clone()
        call(plain, "lagrange_to_coeff", COLS, tab=tables_plain)()
        torch.cuda.synchronize()
        assert torch.equal(out, kept), "the -DAESW_NTT_PASS_LOG=1 build computes another transform"

        # the store floor and the field-product rate of the same session: argument_columns and grand_product at K = 20 / N = 4
        n_sets, u = 4, (1 << K) - 6
        n = pkg.block_capacity(K, n_sets)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        w, kw = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED), ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        theta, beta, gamma = (int.from_bytes(rng.bytes(40), "little") % api.FR_MODULUS for _ in range(3))
        d_theta, d_beta, d_gamma = (torch.from_numpy(api.fr_cell(v)).cuda() for v in (theta, beta, gamma))
        mult, mrep = ctx.lookup_multiplicities(K, n_sets, w, kw, [n])
        assert mrep["misses"] == 0
        a, s_, _prep = ctx.permuted_columns(K, n_sets, mult, n_rows=u)
        inputs, _ = ctx.lookup_inputs(K, n_sets, w, kw)
        table, _trep = ctx.compress_table(d_theta)
        inv, _vrep = ctx.invert_table(table, d_beta, d_gamma)
        grand = api.load_grand_library()
        gz = torch.empty((n_sets, 5, 1 << K, 32), dtype=torch.uint8, device="cuda")
        gclosing = torch.empty((n_sets, 5, 32), dtype=torch.uint8, device="cuda")
        gws = torch.empty(int(grand.aesw_grand_workspace_bytes(K, n_sets)), dtype=torch.uint8, device="cuda")
        grep_ = torch.empty(3, dtype=torch.int64, device="cuda")
        arg_out = torch.empty((n_sets, 5, 1 << K, 32), dtype=torch.uint8, device="cuda")

        def grand_call():
            rc = grand.aesw_grand_product_device(ctx._h, K, n_sets, u, 0, inputs.data_ptr(), a.data_ptr(), s_.data_ptr(), table.data_ptr(), inv.data_ptr(),
                                                 d_beta.data_ptr(), d_gamma.data_ptr(), gz.data_ptr(), gclosing.data_ptr(), gws.data_ptr(), grep_.data_ptr(), ctx._stream())
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

        cands = {}
        for name in NAMES:
            cands[name + " x1"] = call(shipped, name, 1)
            cands[name + " x8"] = call(shipped, name, COLS)
            cands[name + " 8 calls"] = eight(name)
        for pname, lib in masked.items():
            cands["coeff_to_extended x8 " + pname] = call(lib, "coeff_to_extended", COLS)
            if pname != "pass 2":
                cands["lagrange_to_coeff x8 " + pname] = call(lib, "lagrange_to_coeff", COLS)
        cands["plain x1"] = call(plain, "lagrange_to_coeff", 1, tab=tables_plain)
        cands["plain x8"] = call(plain, "lagrange_to_coeff", COLS, tab=tables_plain)
        cands["tables"] = lambda: ctx.ntt_tables(EXT_K, _out=tables)
        cands["argument_columns"] = lambda: ctx.argument_columns(a, table, K, n_sets, out=arg_out)
        cands["grand_product"] = grand_call
        t = dict(zip(cands, _times(torch, [_graph(torch, f) for f in cands.values()])))
        m = {name: ts[REPLAYS // 2] for name, ts in t.items()}
        spread = {name: ts[-1] - ts[0] for name, ts in t.items()}

        size = {"lagrange_to_coeff": K, "coeff_to_lagrange": K, "coeff_to_extended": EXT_K, "extended_to_coeff": EXT_K}
        floor_ns = m["argument_columns"] * 1e6 / (n_sets * 5 << K)  # ns per 32-byte cell stored
        gcells = n_sets * 5 * (u + 1)
        lines = [
            "# The transforms of `libaesw_ntt.so`, measured (`tests/test_perf_ntt.py`, `pytest -m perf -s`)",
            "",
            "K = 20, ext_k = 22 (zeta_sel 1), 1 and 8 columns of seeded canonical cells, every call out of place.  Every figure is the median of",
            "%d graph replays taken in turn with the other candidates after a warm-up replay of each, in one process on one lease.  A pass by" % REPLAYS,
            "itself is the library built with `-DAESW_NTT_PASSES=<mask>`; the plain radix-2 is the library built with `-DAESW_NTT_PASS_LOG=1`",
            "(one stage per pass, %d launches at k = 20, a tile of two cells under 256 threads), with tables of its own." % K,
            "",
            "| what | 1 column | 8 columns | 8 calls of 1 column (spread) | butterflies/s at 8 columns |",
            "|---|---|---|---|---|",
        ]
        for name in NAMES:
            lines.append("| `%s` (2^%d) | %.3f ms | %.3f ms | %.3f ms (%.3f ms) | %.3g |" % (
                name, size[name], m[name + " x1"], m[name + " x8"], m[name + " 8 calls"], spread[name + " 8 calls"], butterflies(size[name], COLS) / m[name + " x8"] * 1e3))
        lines += [
            "",
            "| what | median |",
            "|---|---|",
            "| `lagrange_to_coeff` x8, pass 0 alone (10 stages, bit-reversed load) | %.3f ms |" % m["lagrange_to_coeff x8 pass 0"],
            "| `lagrange_to_coeff` x8, pass 1 alone (10 stages, 1/2^k in the store) | %.3f ms |" % m["lagrange_to_coeff x8 pass 1"],
            "| `coeff_to_extended` x8, pass 0 alone (10 stages, three quarters of the load is padding) | %.3f ms |" % m["coeff_to_extended x8 pass 0"],
            "| `coeff_to_extended` x8, pass 1 alone (10 stages, in place) | %.3f ms |" % m["coeff_to_extended x8 pass 1"],
            "| `coeff_to_extended` x8, pass 2 alone (2 stages, 256 neighbouring sub-transforms a tile) | %.3f ms |" % m["coeff_to_extended x8 pass 2"],
            "| `lagrange_to_coeff` x1, `-DAESW_NTT_PASS_LOG=1` | %.3f ms |" % m["plain x1"],
            "| `lagrange_to_coeff` x8, `-DAESW_NTT_PASS_LOG=1` (spread %.3f ms) | %.3f ms |" % (spread["plain x8"], m["plain x8"]),
            "| `ntt_tables` for max_k = 22 | %.3f ms |" % m["tables"],
            "| `argument_columns` at K = 20 / N = 4 (%d cells stored): the store floor | %.3f ms = %.4f ns per cell |" % (n_sets * 5 << K, m["argument_columns"], floor_ns),
            "| `grand_product` at K = 20 / N = 4 (%d cells of Z, ten field products a cell by 4.20's count) | %.3f ms = %.3g products/s |" % (
                gcells, m["grand_product"], 10 * gcells / m["grand_product"] * 1e3),
            "",
            "Store floor for the transforms' outputs at %.4f ns per cell: 8 x 2^20 cells %.3f ms, 8 x 2^22 cells %.3f ms." % (
                floor_ns, floor_ns * (COLS << K) / 1e6, floor_ns * (COLS << EXT_K) / 1e6),
            "A butterfly is one field product, one sum and one difference (none of the products in stage 1 of a pass); a later pass adds two",
            "products per cell for its load twiddle.",
            "",
            "Condition 1: `lagrange_to_coeff` x8 kept + spread of the plain build <= plain: %.3f + %.3f <= %.3f: %s (%.1f times)." % (
                m["lagrange_to_coeff x8"], spread["plain x8"], m["plain x8"], "held" if m["lagrange_to_coeff x8"] + spread["plain x8"] < m["plain x8"] else "NOT held",
                m["plain x8"] / m["lagrange_to_coeff x8"]),
        ]
        held = {name: m[name + " x8"] <= m[name + " 8 calls"] + spread[name + " 8 calls"] for name in NAMES}
        lines += ["Condition 2, `%s`: 8 columns <= 8 calls + their spread: %.3f <= %.3f + %.3f: %s." % (
            name, m[name + " x8"], m[name + " 8 calls"], spread[name + " 8 calls"], "held" if held[name] else "NOT held") for name in NAMES]
        lines += [
            "",
            "**Not measured:** no `rocprofv3` trace and no counters, so nothing here says what bounds a pass -- the field products, the",
            "scattered 32-byte loads of the first pass, the strided loads and stores of a full later pass, or LDS; the bank-conflict claim of",
            "DESIGN 4.22 was not confirmed by `SQ_LDS_BANK_CONFLICT`; calls in place; the plain and sc1 store modes; other shapes; other leases.",
            "The plain build is a weak comparator: its workgroups keep 256 threads for a tile of two cells.",
            "",
        ]
        print("\n" + "\n".join(lines))
        dst = ROOT / "profiles" / "ntt" / "README.md"
        dst.parent.mkdir(parents=True, exist_ok=True)
        dst.write_text("\n".join(lines))
        assert m["lagrange_to_coeff x8"] + spread["plain x8"] < m["plain x8"], (m["lagrange_to_coeff x8"], spread["plain x8"], m["plain x8"])
        assert all(held.values()), (held, m, spread)
    finally:
        ctx.close()
