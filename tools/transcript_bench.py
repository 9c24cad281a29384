#!/usr/bin/env python3
"""What a challenge costs: the device transcript against the host round trip it replaces (profiles/transcript/README.md).

For n = 1, 12 and 60 commitments (12 = 3N at N = 4), in one process and alternating:

  device   init -> write_points(n) -> squeeze on the stream, nothing waiting in between: as three launches from Python (events
           around a run of them, so the time holds the launches' enqueue where the stream runs dry) and as one captured graph
           replayed (the stream time of the three kernels alone);
  host     what a caller does without the library, from calls that exist without it: synchronise, .cpu() of the [n, 64] points,
           the coordinates out of Montgomery form and the same hash with hashlib, the challenge's cell uploaded (32 bytes),
           synchronise.  Wall time.

Prints one JSON line; --out writes it to a file as well.  The per-compression time is the slope of the graph's time over the
blocks compressed (65 n + 1 bytes hashed, the last block by the squeeze)."""
import argparse
import hashlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

NS = (1, 12, 60)


def host_challenge(torch, api, points, unmont_q):
    """the round trip: download, hash, upload"""
    torch.cuda.synchronize()
    host = points.cpu().numpy()
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
    for row in host:
        x, y = (int.from_bytes(row[i:i + 32].tobytes(), "little") * unmont_q % api.FQ_MODULUS for i in (0, 32))
        h.update(b"\x01" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))
    h.update(b"\x00")
    cell = torch.from_numpy(api.fr_cell(int.from_bytes(h.digest(), "little"))).cuda()
    torch.cuda.synchronize()
    return cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ge.build()
    pkg = ge.load_package()
    api = pkg.api
    ctx = pkg.Context(0)
    unmont_q = pow(1 << 256, -1, api.FQ_MODULUS)
    rng = np.random.default_rng(0x7472)
    result = {"reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "n": {}}
    for n in NS:
        # any canonical coordinates: the time does not depend on whether the point is on the curve
        coords = [int.from_bytes(rng.bytes(31), "little") for _ in range(2 * n)]
        points = torch.from_numpy(np.stack([api.fq_cell(v) for v in coords]).reshape(n, 64)).cuda()
        t = ctx.transcript(32 * n)
        challenge = torch.empty(32, dtype=torch.uint8, device="cuda")

        def chain():
            t.reset()
            t.write_points(points)
            t.squeeze(out=challenge)

        chain()
        expected = host_challenge(torch, api, points, unmont_q)
        assert torch.equal(challenge, expected), "the device and the host disagree at n = %d" % n
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            chain()
        torch.cuda.synchronize()
        launches, replays, host = [], [], []
        for _ in range(args.rounds):  # the three ways alternate within a round
            for what, into in ((chain, launches), (graph.replay, replays)):
                for _warm in range(10):
                    what()
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                begin.record()
                for _rep in range(args.reps):
                    what()
                end.record()
                torch.cuda.synchronize()
                into.append(begin.elapsed_time(end) * 1e3 / args.reps)
            walls = []
            for _rep in range(max(args.reps // 4, 10)):
                t0 = time.perf_counter()
                host_challenge(torch, api, points, unmont_q)
                walls.append((time.perf_counter() - t0) * 1e6)
            host.append(statistics.median(walls))
        blocks = -(-(65 * n + 1) // 128)
        result["n"][str(n)] = {"blocks": blocks, "device_launches_us": [round(v, 2) for v in launches], "device_graph_us": [round(v, 2) for v in replays],
                               "host_round_trip_us": [round(v, 2) for v in host]}
    lo, hi = result["n"][str(NS[0])], result["n"][str(NS[-1])]
    result["per_compression_us"] = round((statistics.median(hi["device_graph_us"]) - statistics.median(lo["device_graph_us"])) / (hi["blocks"] - lo["blocks"]), 3)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
