#!/usr/bin/env python3
"""What the quotient's segments cost (profiles/vanish/README.md), by the method of profiles/open/README.md: medians of 21 graph
replays taken in turn after a warm-up replay of each, in one process.  Default: K = 20, ext_k = 22, N = 4, chunk_len 3.

  head, perm, lookup, divide   one call of each segment kind (perm: a set of chunk_len columns)
  fold                         the whole fold: HEAD, every PERM, every LOOKUP, the division, one linear chain
  lookup_lds, fold_lds         the same with the lookup kernel of a variant built with -DAESW_VANISH_LDS=1, which stages Z[next] and
                               A'[prev] through LDS where the shipped kernel reads them again through the cache; the two builds
                               are held to the same cells before either is timed
  grand_product                the yardstick of DESIGN.md 4.23: the lookup grand product at K / N, ten field products a cell of Z

Every segment reads the same seeded buffer of 30 extended columns -- the largest segment's, LOOKUP's -- as a caller does who
extends a group, folds it and uses the buffer again: the time of a field product does not depend on the cells.  A rate is priced
by a segment's share of quot_products_per_row (csrc/aesw_vanish.h's vanish_segment_products; 436 a row at N = 4, 4.23's count), not
by the products a call runs, which the line gives next to it.  The bytes of the fold's tensors -- that buffer, acc, the tables,
the scalars block -- are computed from their shapes; what the allocator held before the yardstick's buffers is given beside them.  Prints one JSON line; --out writes it
to a file as well."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

REPLAYS = 21


def captured(torch, fn):
    fn()  # first launches outside the graph
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    torch.cuda.synchronize()
    return graph


def medians(torch, graphs):
    """name -> (median ms, spread ms) over REPLAYS replays taken in turn"""
    times = {name: [] for name in graphs}
    for graph in graphs.values():
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(REPLAYS):
        for name, graph in graphs.items():
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            graph.replay()
            end.record()
            torch.cuda.synchronize()
            times[name].append(begin.elapsed_time(end))
    return {name: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--ext-k", type=int, default=22)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--chunk-len", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ge.build()
    pkg = ge.load_package()
    api = pkg.api
    ctx = pkg.Context(0)
    k, ext_k, n_sets, chunk_len = args.k, args.ext_k, args.sets, args.chunk_len
    rows, n_rows = 1 << ext_k, (1 << k) - 6
    dev = torch.device("cuda", 0)
    perm_sets, cols = api.permutation_sets(n_sets, chunk_len), 3 * n_sets + 2
    gen = torch.Generator(device=dev).manual_seed(0x766e)
    buf = torch.randint(0, 256, (30, rows, 32), dtype=torch.uint8, device=dev, generator=gen)
    buf[:, :, 31] &= 0x1F  # canonical cells: the top byte keeps them below r
    rng = np.random.default_rng(0x766e)
    theta, beta, gamma, y = (int.from_bytes(rng.bytes(40), "little") % api.FR_MODULUS for _ in range(4))
    tables = ctx.vanishing_tables(k, ext_k, 1)
    scalars = ctx.vanishing_scalars(n_sets, chunk_len, theta, beta, gamma, y)
    lib = api.load_vanish_library()
    acc = torch.empty((rows, 32), dtype=torch.uint8, device=dev)
    if perm_sets > 24:
        raise SystemExit("more permutation sets than the buffer holds columns for")
    shape, p = (k, ext_k, n_sets, chunk_len, n_rows), lambda t: t.data_ptr()  # noqa: E731

    def check(rc):
        assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

    # the C entry points over slices of the one buffer: inputs may overlap one another, only acc is written
    def head():
        check(lib.aesw_vanish_head_device(ctx._h, *shape, p(buf[29]), p(buf[24:26]), p(buf[:perm_sets]), p(buf[26:29]), p(scalars), p(acc), ctx._stream()))

    def perm(s):
        check(lib.aesw_vanish_perm_device(ctx._h, *shape, s, p(buf), p(buf[8:]), p(buf[16]), p(buf[26:29]), p(tables), p(scalars), p(acc), p(acc), ctx._stream()))

    def lookup(s, lib=lib):
        check(lib.aesw_vanish_lookup_device(ctx._h, *shape, s, p(buf[0:3]), p(buf[3:8]), p(buf[8:12]), p(buf[12:17]), p(buf[17:22]), p(buf[22:27]), p(buf[27:30]), p(scalars),
                                            p(acc), p(acc), ctx._stream()))

    def divide():
        check(lib.aesw_vanish_divide_device(ctx._h, k, ext_k, p(tables), p(acc), p(acc), ctx._stream()))

    def fold(lookup_lib=lib):
        head()
        for s in range(perm_sets):
            perm(s)
        for s in range(n_sets):
            lookup(s, lookup_lib)
        divide()

    staged = api.load_vanish_library(ge._load_build().build_vanishing("vanish", extra_flags=["-DAESW_VANISH_LDS=1"], out="libaesw_vanish_lds.so"))
    fold()
    kept = acc.clone()
    fold(staged)
    torch.cuda.synchronize()
    assert torch.equal(acc, kept), "the -DAESW_VANISH_LDS=1 build folds another quotient"

    torch.cuda.synchronize()
    held_before = torch.cuda.memory_allocated()
    graphs = {"head": captured(torch, head), "perm": captured(torch, lambda: perm(0)), "lookup": captured(torch, lambda: lookup(0)), "divide": captured(torch, divide),
              "fold": captured(torch, fold), "lookup_lds": captured(torch, lambda: lookup(0, staged)), "fold_lds": captured(torch, lambda: fold(staged))}

    # the yardstick: grand_product at K / N, as tests/test_perf_ntt.py takes it
    n = pkg.block_capacity(k, n_sets)
    key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).to(dev)
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).to(dev)
    w, kw = ctx.encrypt_witness(pt, key, layout=pkg.LAYOUT_PACKED), ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
    d_theta, d_beta, d_gamma = (torch.from_numpy(api.fr_cell(v)).to(dev) for v in (theta, beta, gamma))
    mult, _mrep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n])
    a, s_, _prep = ctx.permuted_columns(k, n_sets, mult, n_rows=n_rows)
    inputs, _ = ctx.lookup_inputs(k, n_sets, w, kw)
    table, _trep = ctx.compress_table(d_theta)
    inv, _vrep = ctx.invert_table(table, d_beta, d_gamma)
    grand = api.load_grand_library()
    gz = torch.empty((n_sets, 5, 1 << k, 32), dtype=torch.uint8, device=dev)
    gclosing = torch.empty((n_sets, 5, 32), dtype=torch.uint8, device=dev)
    gws = torch.empty(int(grand.aesw_grand_workspace_bytes(k, n_sets)), dtype=torch.uint8, device=dev)
    grep_ = torch.empty(3, dtype=torch.int64, device=dev)

    def grand_call():
        rc = grand.aesw_grand_product_device(ctx._h, k, n_sets, n_rows, 0, inputs.data_ptr(), a.data_ptr(), s_.data_ptr(), table.data_ptr(), inv.data_ptr(),
                                             d_beta.data_ptr(), d_gamma.data_ptr(), gz.data_ptr(), gclosing.data_ptr(), gws.data_ptr(), grep_.data_ptr(), ctx._stream())
        assert rc == 0, ctx._lib.aesw_last_error(ctx._h)

    graphs["grand_product"] = captured(torch, grand_call)
    ms = medians(torch, graphs)
    # priced in quot_products_per_row's own count (csrc/aesw_vanish.h's shares; 4.23's yardstick): a PERM and a LOOKUP that are not the
    # first, which carry nothing the row shares; `run`: what a call runs, the price of the cut included
    width = min(chunk_len, cols)
    per_row = {"head": 2 * perm_sets + 4, "perm": 4 * width + 2, "lookup": 87, "divide": 1, "fold": 12 + 4 * perm_sets + 4 * cols + 87 * n_sets}
    run = {"head": per_row["head"], "perm": 4 * width + 3, "lookup": 90, "divide": 1, "fold": per_row["fold"] + perm_sets + 3 * n_sets - 7}
    per_row.update(lookup_lds=per_row["lookup"], fold_lds=per_row["fold"])
    rate = {name: round(per_row[name] * rows / (ms[name][0] * 1e-3), 0) for name in per_row}
    grand_rate = 10 * 5 * n_sets * (1 << k) / (ms["grand_product"][0] * 1e-3)
    computed = sum(t.numel() * t.element_size() for t in (buf, acc, tables, scalars))
    result = {"device": torch.cuda.get_device_name(0), "k": k, "ext_k": ext_k, "n_sets": n_sets, "chunk_len": chunk_len, "replays": REPLAYS, "ms": ms,
              "products_per_row": per_row, "products_run_per_row": run, "products_per_s": rate, "grand_product_products_per_s": round(grand_rate, 0),
              "fold_rate_over_grand_product": round(rate["fold"] / grand_rate, 3), "lookup_rate_over_grand_product": round(rate["lookup"] / grand_rate, 3),
              "lookup_lds_over_cache_time": round(ms["lookup_lds"][0] / ms["lookup"][0], 4), "fold_lds_over_cache_time": round(ms["fold_lds"][0] / ms["fold"][0], 4),
              "fold_tensors_bytes_computed": computed, "allocated_bytes_before_the_yardstick": held_before,
              "all_columns_bytes_computed": 32 * rows * (sum((3 * n_sets + 1, 2, 5 * n_sets, 4, cols, perm_sets, 5 * n_sets, 5 * n_sets, 5 * n_sets, 3)) + 1)}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
