"""Timing of plookup's permuted columns from the lookup multiplicities (libaesw_perm.so).

    python tools/perm_bench.py [--reps 21] [--k 20] [--sets 4] [--out FILE]

One process, one circuit at K / N filled to its capacity, its histograms from the accumulator; every figure the median of --reps
graph replays taken in turn with the other candidates of its group.
  * build: aesw_perm_build_device over all 5 N arguments (n_rows = 2^K) for three histograms -- the circuit's own, the circuit
    of identical blocks (a few Xor bins hold every lookup: runs that span hundreds of workgroups) and the empty one (every
    position in the all-zero run: the store stream alone) -- next to a fill_ of the bytes it writes and to torch.sort over the
    5 N shuffled input columns, which is what the count replaces and builds no S';
  * gather: aesw_perm_gather_fr_device over one argument's and over all arguments' A' against aesw_expand_fr_device over as
    many cells.
One JSON line at the end (and into --out)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.acc_bench import graph_of, in_turn  # noqa: E402  (the capture and the clock)


def histograms(torch, pkg, ctx, k, n_sets, identical):
    n = pkg.block_capacity(k, n_sets)
    rng = np.random.default_rng(k)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if identical:
        pt[:] = pt[0]
    key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    acc = ctx.multiplicity_accumulator(k, n_sets).reset()
    acc.add(0, ctx.encrypt_witness(torch.from_numpy(pt).cuda(), key, layout=pkg.LAYOUT_PACKED))
    acc.add_key(ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False))
    assert acc.report()["misses"] == 0
    return n, acc.histograms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    arg = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    lib = pkg.api.load_perm_library()
    k, n_sets, u = arg.k, arg.sets, 1 << arg.k
    n_args = 5 * n_sets
    n, real = histograms(torch, pkg, ctx, k, n_sets, False)
    _n, same = histograms(torch, pkg, ctx, k, n_sets, True)
    mults = {"circuit": real, "identical_blocks": same, "empty": torch.zeros_like(real)}
    shape = (n_sets, 5, u)
    a, s = torch.empty(shape, dtype=torch.int32, device="cuda"), torch.empty(shape, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.aesw_perm_workspace_bytes(n_sets)), dtype=torch.uint8, device="cuda")
    rep = torch.empty(3, dtype=torch.int64, device="cuda")

    def build(mult):
        def f():
            rc = lib.aesw_perm_build_device(ctx._h, k, n_sets, u, 0, mult.data_ptr(), a.data_ptr(), s.data_ptr(), ws.data_ptr(), rep.data_ptr(), ctx._stream())
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
        return f

    build(real)()
    torch.cuda.synchronize()
    inputs = torch.stack([col[torch.randperm(u, device="cuda")] for col in a.view(n_args, u)]).contiguous()
    sorted_out, order_out = torch.empty_like(inputs), torch.empty(inputs.shape, dtype=torch.int64, device="cuda")
    graphs = [graph_of(torch, build(m)) for m in mults.values()]
    graphs.append(graph_of(torch, lambda: torch.sort(inputs, dim=1, out=(sorted_out, order_out))))
    graphs[0].replay()  # the last build captured was the empty histogram's
    torch.cuda.synchronize()
    assert torch.equal(sorted_out, a.view(n_args, u)), "the sort and the count disagree on A'"
    graphs.append(graph_of(torch, lambda: (a.fill_(1), s.fill_(2))))
    ts = in_turn(torch, graphs, arg.reps)
    written = 2 * n_args * u * 4
    res = {"k": k, "n_sets": n_sets, "blocks": n, "arguments": n_args, "written_bytes": written,
           "build_us": {name: round(t * 1e3, 1) for name, t in zip(mults, ts)}, "sort_us": round(ts[3] * 1e3, 1), "fill_us": round(ts[4] * 1e3, 1),
           "build_tb_per_s": round(written / ts[0] / 1e9, 2), "fill_tb_per_s": round(written / ts[4] / 1e9, 2), "build_over_sort": round(ts[0] / ts[3], 4)}
    print("K=%d N=%d, %d blocks, %d arguments:" % (k, n_sets, n, n_args), res)

    graphs[0].replay()  # a holds the circuit's columns again
    table = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (66561, 32), dtype=np.uint8)).cuda()
    gather = {}
    for name, cells in (("one_argument", u), ("all_arguments", n_args * u)):
        index, out = a.view(-1)[:cells], torch.empty((cells, 32), dtype=torch.uint8, device="cuda")
        bytes_in = torch.randint(0, 256, (cells,), dtype=torch.uint8, device="cuda")
        tg, te = in_turn(torch, [graph_of(torch, lambda: ctx.gather_fr(index, table, out=out)), graph_of(torch, lambda: ctx.expand_fr(bytes_in, out=out))], arg.reps)
        gather[name] = {"cells": cells, "gather_us": round(tg * 1e3, 1), "expand_fr_us": round(te * 1e3, 1), "gather_tb_per_s": round(cells * 32 / tg / 1e9, 2),
                        "expand_fr_tb_per_s": round(cells * 32 / te / 1e9, 2)}
        del out
    res["gather"] = gather
    print("gather_fr against expand_fr:", gather)
    ctx.close()
    line = json.dumps({"perm_bench": res})
    print(line)
    if arg.out:
        Path(arg.out).parent.mkdir(parents=True, exist_ok=True)
        Path(arg.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
