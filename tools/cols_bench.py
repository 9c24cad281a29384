#!/usr/bin/env python3
"""Times the column checker (Context.check_columns, libaesw_cols.so) in one process: byte form, Fr form, the slab checker
(Context.check_circuits on DENSE slabs of the same batch) and the Fr assemble launch that wrote the same bytes, alternating
over the same buffers, median of five.  Prints one JSON line per shape; --out writes them to a file.

  python tools/cols_bench.py [--out profiles/cols/cols_bench_run1.json] [--shapes 20,5,4 14,1,4096]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(pkg, ctx, k, n_sets, nc, reps=5):
    import numpy as np
    import torch
    cap = pkg.block_capacity(k, n_sets)
    counts = [cap] * nc
    n = cap * nc
    rng = np.random.default_rng(k * 1000 + nc)
    keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    offs = pkg.circuit_offsets(k, n_sets, counts, n)
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    kw = ctx.key_schedule_witness(keys, pkg.LAYOUT_DENSE, want_rk=False)
    per_block = torch.repeat_interleave(keys, torch.as_tensor(counts, dtype=torch.int64, device="cuda"), dim=0)
    wit = ctx.encrypt_witness(pt, per_block, pkg.LAYOUT_DENSE, want_ct=True)
    del per_block
    adv_b = ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=False, layout=pkg.LAYOUT_DENSE, n_blocks=n, _offsets=d_offs)
    adv_f = ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=True, layout=pkg.LAYOUT_DENSE, n_blocks=n, _offsets=d_offs)
    torch.cuda.synchronize()
    runs = {
        "slab_check_dense": lambda: ctx.check_circuits(k, n_sets, pt, keys, wit, kw, counts, layout=pkg.LAYOUT_DENSE, ct=wit.ct, sync=False, _offsets=d_offs),
        "cols_check_bytes": lambda: ctx.check_columns(k, n_sets, pt, keys, adv_b, counts, ct=wit.ct, sync=False, _offsets=d_offs),
        "cols_check_fr": lambda: ctx.check_columns(k, n_sets, pt, keys, adv_f, counts, ct=wit.ct, sync=False, _offsets=d_offs),
        "assemble_fr": lambda: ctx.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=True, layout=pkg.LAYOUT_DENSE, n_blocks=n,
                                                            out=adv_f, _offsets=d_offs),
    }
    for name in ("cols_check_bytes", "cols_check_fr"):
        rep = pkg.api.cols_report_dict(runs[name]())
        assert rep["satisfied"] and rep["blocks"] == n, (name, rep)
    times = {name: [] for name in runs}
    for _ in range(reps + 1):  # the first turn warms up
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    med = {name: statistics.median(v[1:]) for name, v in times.items()}
    cells = nc * (3 * n_sets + 1) << k
    return {"k": k, "n_sets": n_sets, "circuits": nc, "blocks": n, "cells": cells, "us_median_of_%d" % reps: med,
            "us_all": {name: v[1:] for name, v in times.items()},
            "bytes_over_slab": med["cols_check_bytes"] / med["slab_check_dense"],
            "fr_read_TBps": cells * 32 / med["cols_check_fr"] / 1e6,
            "bytes_read_GBps": cells / med["cols_check_bytes"] / 1e3,
            "fr_check_over_assemble_fr": med["cols_check_fr"] / med["assemble_fr"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", nargs="*", default=["20,5,4", "14,1,4096"])
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    rows = []
    for s in a.shapes:
        k, n_sets, nc = (int(v) for v in s.split(","))
        rows.append(measure(pkg, ctx, k, n_sets, nc))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
