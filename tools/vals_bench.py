#!/usr/bin/env python3
"""Times the values checker (Context.check_values, libaesw_vals.so) against the PACKED slab checker (Context.check_witness) over
the witnesses of the same inputs, in one process, alternating, median of five.  Prints one JSON line per case; --out writes
them to a file.

  python tools/vals_bench.py [--out profiles/vals/vals_bench_run1.json] [--cases 1048576,1 65536,0]      (blocks, per_block_keys)"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(pkg, ctx, n, pbk, reps=5):
    import numpy as np
    import torch
    rng = np.random.default_rng(n + pbk)
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    keys = torch.from_numpy(rng.integers(0, 256, (n, 16) if pbk else 16, dtype=np.uint8)).cuda()
    v = ctx.encrypt_witness(pt, keys, layout=pkg.LAYOUT_VALUES, want_ct=True, key_slab=True)
    p = ctx.encrypt_witness(pt, keys, layout=pkg.LAYOUT_PACKED, want_ct=True, key_slab=True)
    torch.cuda.synchronize()
    runs = {
        "values_check": lambda: ctx.check_values(pt, keys, v, v.key, ct=v.ct, sync=False),
        "packed_check": lambda: ctx.check_witness(pt, keys, p, p.key, layout=pkg.LAYOUT_PACKED, ct=p.ct, sync=False),
    }
    for name, fn in runs.items():
        rep = pkg.api.check_report_dict(fn())
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
    med = {name: statistics.median(t[1:]) for name, t in times.items()}
    key_bytes = 936 * (n if pbk else 1)
    read = {"values_check": n * (448 + 608 + 32) + key_bytes + 16 * (n if pbk else 1), "packed_check": n * (3024 + 32) + key_bytes + 16 * (n if pbk else 1)}
    return {"blocks": n, "per_block_keys": bool(pbk), "us_median_of_%d" % reps: med, "us_all": {name: t[1:] for name, t in times.items()},
            "values_over_packed": med["values_check"] / med["packed_check"],
            "blocks_per_s": {name: n / med[name] * 1e6 for name in runs},
            "read_GBps": {name: read[name] / med[name] / 1e3 for name in runs}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--cases", nargs="*", default=["1048576,1", "65536,0", "65536,1", "1048576,0"])
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    rows = []
    for s in a.cases:
        n, pbk = (int(x) for x in s.split(","))
        rows.append(measure(pkg, ctx, n, pbk))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
