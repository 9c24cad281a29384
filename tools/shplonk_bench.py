#!/usr/bin/env python3
"""What a set's quotient costs: the fused path of libaesw_shplonk.so against the same polynomial composed from the calls that
exist without it (profiles/shplonk/README.md), by the method of profiles/open/README.md: medians of 21 graph replays taken in
turn after a warm-up replay of each, in one process.

  fused     combine_columns (N_i = sum_j y^j P_ij - R_i) + set_quotient (v^i Q_i by partial fractions, three passes over N_i)
  composed  fold_columns over the reversed columns under y (acc y + col gives sum_j y^j P_ij with the columns reversed), then
            t divide_columns -- one per point of the set, three passes each -- and a scaling fold per point into the result
            (fold_columns as acc * w + column: quotient_s * w_s + the sum so far); the low cells -R_i are left out of the
            composed path, which favours it

and the whole open_shplonk stage for the chain test's plan (three sets over the rotations 0, 1, -1) at --stage-k, commitments and
transcript included.  Default: one set of 8 columns, t = 3, K = 20.  Prints one JSON line; --out writes it to a file as well."""
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


def seeded_cells(rng, *shape):
    """canonical cells: the top byte keeps them below r"""
    cells = rng.integers(0, 256, shape + (32,), dtype=np.uint8)
    cells[..., 31] &= 0x1F
    return cells


def captured(torch, fn):
    fn()  # allocations and first launches outside the graph
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
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--points", type=int, default=3)
    ap.add_argument("--stage-k", type=int, default=17)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ge.build()
    pkg = ge.load_package()
    api = pkg.api
    ctx = pkg.Context(0)
    rng = np.random.default_rng(0x7368)
    k, m, t, n = args.k, args.cols, args.points, 1 << args.k
    dev = torch.device("cuda", 0)
    columns = torch.from_numpy(seeded_cells(rng, m, n)).to(dev)
    reversed_columns = columns.flip(0).contiguous()
    points = torch.from_numpy(seeded_cells(rng, t)).to(dev)
    y, v = (torch.from_numpy(seeded_cells(rng)).to(dev) for _ in range(2))
    plan = api.multiopen_plan([(c, r) for c in range(m) for r in range(t)])
    evals = ctx.evaluate_columns(columns, k, points).reshape(m * t, 32).contiguous()
    scalars, report = ctx.shplonk_prepare(plan, points, evals, y, v)
    numer, out, rem = (torch.empty(shape, dtype=torch.uint8, device=dev) for shape in ((n, 32), (n, 32), (8, 32)))
    ws = torch.empty(int(api.load_shplonk_library().aesw_shplonk_workspace_bytes(k)), dtype=torch.uint8, device=dev)
    y_pow, neg_r = ctx.shplonk_table(scalars, "y_pow", cells=m), ctx.shplonk_table(scalars, "neg_r", 0, t)
    weights = ctx.shplonk_table(scalars, "vw", 0, t)

    def fused():
        ctx.combine_columns(columns, k, y_pow, low=neg_r, out=numer)
        ctx.set_quotient(numer, k, 0, points, scalars, report, out=out, _rem=rem, _workspace=ws)

    folded, quot, one_rem = (torch.empty(shape, dtype=torch.uint8, device=dev) for shape in ((n, 32), (t, n, 32), (32,)))
    sums = [torch.empty((n, 32), dtype=torch.uint8, device=dev) for _ in range(2)]
    open_ws = torch.empty(int(api.load_open_library().aesw_open_workspace_bytes(k, 1, 1)), dtype=torch.uint8, device=dev)
    zero = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

    def composed():
        ctx.fold_columns(reversed_columns, k, y, out=folded)
        for s in range(t):
            ctx.divide_columns(folded, k, points[s], out=quot[s], _rem=one_rem, _workspace=open_ws)
        for s in range(t):  # a fold computes acc * v + column: quot_s * w_s + the sum so far, between two buffers
            ctx.fold_columns(sums[(s + 1) % 2] if s else zero, k, weights[s], acc=quot[s], out=sums[s % 2])

    graphs = {"fused": captured(torch, fused), "composed": captured(torch, composed), "combine": captured(torch, lambda: ctx.combine_columns(columns, k, y_pow, low=neg_r, out=numer)),
              "set_quotient": captured(torch, lambda: ctx.set_quotient(numer, k, 0, points, scalars, report, out=out, _rem=rem, _workspace=ws))}
    result = {"device": torch.cuda.get_device_name(0), "k": k, "cols": m, "points": t, "replays": REPLAYS, "ms": medians(torch, graphs)}

    # the whole stage for the chain test's plan
    sk, sn = args.stage_k, 1 << args.stage_k
    stage_plan = api.multiopen_plan([("advice", 0), ("z", 0), ("z", 1), ("z2", 0), ("z2", 1), ("z2", -1), ("advice2", -1), ("advice2", 0), ("advice2", 1)])
    stage_columns = [torch.from_numpy(seeded_cells(rng, len(cols), sn)).to(dev) for _idx, cols in stage_plan.sets]
    stage_points = torch.from_numpy(api.rotated_points(0x1234567, sk, stage_plan.rotations)).to(dev)
    stage_evals = torch.cat([ctx.evaluate_columns(cols, sk, stage_points[list(idx)]).reshape(-1, 32) for (idx, _c), cols in zip(stage_plan.sets, stage_columns)]).contiguous()
    basis = torch.from_numpy(seeded_cells(rng, sn, 2).reshape(sn, 64)).to(dev)  # any canonical coordinates: the time does not depend on the curve
    transcript = ctx.transcript(64)
    points_out, stage_report = torch.empty((2, 64), dtype=torch.uint8, device=dev), torch.empty(8, dtype=torch.int64, device=dev)

    def stage():
        transcript.reset()
        ctx.open_shplonk(stage_plan, stage_columns, stage_evals, stage_points, transcript, basis, out=points_out, _report=stage_report)

    result["stage"] = {"k": sk, "sets": [[len(idx), len(cols)] for idx, cols in stage_plan.sets], "ms": medians(torch, {"open_shplonk": captured(torch, stage)})["open_shplonk"]}
    torch.cuda.synchronize()
    result["stage"]["report"] = {key: val for key, val in api.shplonk_report_dict(stage_report).items() if key != "last_remainder"}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
