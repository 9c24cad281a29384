"""Device groups against a plain context: aesw_encrypt_witness and aesw_encrypt_witness_stream, packed layout, per-block keys.

    python tools/group_bench.py [--log2 24] [--reps 3] [--out FILE]

Host path: page-locked input and page-locked x / y / z columns (aesw_host_alloc, direct DMA).  The columns of 2^24 blocks are
50.7 GB; when the host cannot spare twice that the batch is halved until it can, and the JSON says how many blocks were used.
Stream: a consumer that only returns (the link and the pipeline, not the host's assign loop).  Configurations, interleaved call
by call in an order that rotates, so that drift hits them alike: a plain Context(0), a second plain Context(0) (the control:
how far two plain contexts differ), a Group([0]) and a Group([0, 0]) (two members on one GPU and one link).  Median of --reps
calls each, after one untimed call that sizes every context's buffers."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def mem_available():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    lay = pkg.LAYOUT_PACKED
    per_block = sum(pkg.column_stride(lay, c) for c in range(3))
    n_stream = 1 << a.log2
    n_host = n_stream
    while n_host > (1 << 16) and 2 * n_host * (per_block + 32) > mem_available():
        n_host //= 2
    rng = np.random.default_rng(0x6A0)
    hpt = pkg.api.host_alloc(n_stream * 16).reshape(n_stream, 16)
    hkeys = pkg.api.host_alloc(n_stream * 16).reshape(n_stream, 16)
    hpt[:] = rng.integers(0, 256, (n_stream, 16), dtype=np.uint8)
    hkeys[:] = rng.integers(0, 256, (n_stream, 16), dtype=np.uint8)
    cols = [pkg.api.host_alloc(n_host * pkg.column_stride(lay, c)) for c in range(3)]
    # context_b: a second plain context, the control for what differs between any two contexts (their device scratch, ...)
    configs = {"context": pkg.Context(0), "context_b": pkg.Context(0), "group_0": pkg.Group([0]), "group_0_0": pkg.Group([0, 0])}
    res = {"layout": "packed", "keys": "per-block", "host": {"blocks": n_host, "destination": "aesw_host_alloc"},
           "stream": {"blocks": n_stream, "consumer": "returns at once"}}

    def host(c):
        c.encrypt_witness_host(hpt[:n_host], hkeys[:n_host], layout=lay, out_cols=cols)

    def stream(c):
        c.encrypt_witness_stream(hpt, hkeys, lambda *args: 0, layout=lay)

    for what, fn, n in (("host", host, n_host), ("stream", stream, n_stream)):
        times = {k: [] for k in configs}
        for c in configs.values():
            fn(c)  # sizes the buffers, untimed
        names = list(configs)
        for r in range(a.reps):
            for k in names[r % len(names):] + names[:r % len(names)]:  # the order rotates from call to call
                c = configs[k]
                t0 = time.perf_counter()
                fn(c)
                times[k].append(time.perf_counter() - t0)
        for k, ts in times.items():
            dt = sorted(ts)[len(ts) // 2]
            res[what][k] = {"ms": round(dt * 1e3, 1), "GBps_to_host": round(n * per_block / dt / 1e9, 2),
                            "spread_pct": round((max(ts) - min(ts)) / dt * 100, 1), "ms_all": [round(t * 1e3, 1) for t in ts]}
    # the parity the tests hold at small sizes, once at this size: the group's columns equal the context's
    host(configs["context"])
    ref = [np.array(c, copy=True) for c in cols]
    for c in cols:
        c[:] = 0
    host(configs["group_0_0"])
    res["host"]["group_0_0_equals_context"] = all(np.array_equal(r, c) for r, c in zip(ref, cols))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    for c in configs.values():
        c.close()
    for b in cols + [hpt.reshape(-1), hkeys.reshape(-1)]:
        pkg.api.host_free(b)
    return 0


if __name__ == "__main__":
    sys.exit(main())
