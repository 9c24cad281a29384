#!/usr/bin/env python3
"""What blinding costs on the device (profiles/blind/README.md), at K = 20 in one process and one session:

  fill     blind_rows at first_row = 0 over --fill-cols columns: every row a blinding cell, so the figure is cells a second of the
           fill kernel (two Blake2b compressions and two field products a cell);
  tail     commit_tail for 12 columns of 6 tail rows: one wave a column, 254 doublings and additions a lane;
  commit   commit_blinded_bytes over 12 byte columns with their tails -- commit_columns over the bytes, one 8-bit window, then
           commit_tail -- against commit_columns over the same 12 columns expanded to Fr cells with blind_rows applied, 32 windows.
           The two give the same 12 commitments (asserted); the ratio of their times is what the byte path keeps of the window
           count's 32.

The basis is the generator at every row: the complete addition law costs the same for any pair of points.  Times are medians over
--rounds rounds of --reps calls between two events.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

COLS, TAIL = 12, 6


def timed(torch, what, reps, rounds):
    """the median over `rounds` of the milliseconds a call of `what` takes, `reps` calls between two events"""
    out = []
    for _ in range(rounds):
        what()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        for _rep in range(reps):
            what()
        end.record()
        torch.cuda.synchronize()
        out.append(begin.elapsed_time(end) / reps)
    return statistics.median(out), [round(v, 4) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--fill-cols", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ge.build()
    pkg = ge.load_package()
    api = pkg.api
    ctx = pkg.Context(0)
    k, n = args.k, 1 << args.k
    first_row = n - TAIL
    canonical = np.zeros((n, 64), np.uint8)
    canonical[:, 0], canonical[:, 32] = 1, 2  # G = (1, 2)
    basis = ctx.msm_basis(canonical)
    seed = ctx.blinding_seed(bytes(range(32)))
    result = {"k": k, "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "fr_store_mode": ctx.get_option("fr_store_mode")}

    fill = torch.empty((args.fill_cols, n, 32), dtype=torch.uint8, device="cuda")
    ms, runs = timed(torch, lambda: ctx.blind_rows(fill, k, 0, seed, 1), args.reps, args.rounds)
    result["fill"] = {"columns": args.fill_cols, "ms": round(ms, 4), "runs_ms": runs, "cells_per_s": round(args.fill_cols * n / (ms * 1e-3), 1)}
    del fill

    body = torch.from_numpy(np.random.default_rng(0x62656e6368).integers(0, 256, (COLS, n), dtype=np.uint8)).cuda()
    body[:, first_row:] = 0
    tail = ctx.blinding_tail(k, COLS, first_row, seed, 2)
    commitments = ctx.commit_columns(body, basis)
    ms, runs = timed(torch, lambda: ctx.commit_tail(tail, k, first_row, basis, commitments), args.reps, args.rounds)
    result["tail"] = {"columns": COLS, "rows": TAIL, "ms": round(ms, 4), "runs_ms": runs}

    lib = api.load_msm_library()
    ws_bytes = torch.empty(int(lib.aesw_msm_workspace_bytes(k, COLS, api.MSM_BYTES, 0)), dtype=torch.uint8, device="cuda")
    out_bytes = torch.empty((COLS, 64), dtype=torch.uint8, device="cuda")
    plain_ms, plain_runs = timed(torch, lambda: ctx.commit_columns(body, basis, out=out_bytes, _workspace=ws_bytes), args.reps, args.rounds)
    blinded_ms, blinded_runs = timed(torch, lambda: ctx.commit_blinded_bytes(body, tail, k, first_row, basis, out=out_bytes, _workspace=ws_bytes), args.reps, args.rounds)
    mont = torch.from_numpy(np.stack([api.fr_cell(v) for v in range(256)])).cuda()
    cells = mont[body.long()].contiguous()
    ctx.blind_rows(cells, k, first_row, seed, 2)
    ws_cells = torch.empty(int(lib.aesw_msm_workspace_bytes(k, COLS, api.MSM_FR, 0)), dtype=torch.uint8, device="cuda")
    out_cells = torch.empty((COLS, 64), dtype=torch.uint8, device="cuda")
    cells_ms, cells_runs = timed(torch, lambda: ctx.commit_columns(cells, basis, out=out_cells, _workspace=ws_cells), max(args.reps // 2, 1), args.rounds)
    torch.cuda.synchronize()
    assert torch.equal(out_bytes, out_cells), "the blinded byte commitment and the commitment of the blinded cells differ"
    result["commit"] = {"columns": COLS, "rows": TAIL, "bytes_alone_ms": round(plain_ms, 4), "bytes_alone_runs_ms": plain_runs, "blinded_bytes_ms": round(blinded_ms, 4),
                        "blinded_bytes_runs_ms": blinded_runs, "blinded_cells_ms": round(cells_ms, 4), "blinded_cells_runs_ms": cells_runs,
                        "cells_over_blinded_bytes": round(cells_ms / blinded_ms, 2), "cells_over_bytes_alone": round(cells_ms / plain_ms, 2)}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
