"""Timing of the multiplicity accumulator (libaesw_acc.so) against the one-shot count of libaesw_mult.so.

    python tools/acc_bench.py [--reps 21] [--out FILE]

One process, PACKED slabs, every figure the median of --reps graph replays taken in turn with the other candidates of its group.
  * chunk size: one circuit at K = 24 / N = 4 filled to its capacity, reset + one add + add_key with the blocks per pair of
    workgroups forced to 64, 128, 256, 512, 1 024, 2 048 and left to the default rule;
  * one circuit: the default against aesw_mult_count_device (AUTO and PRIVATE forced) over the same slabs, at K = 24 / N = 4 and
    K = 20 / N = 4;
  * the stream shape: the K = 24 circuit added in runs of 2^15 blocks (the default chunk_blocks of the host stream), one add
    per run, against the one add over the whole circuit.
One JSON line at the end (and into --out)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CHUNKS = (64, 128, 256, 512, 1024, 2048, 0)
STREAM_BLOCKS = 1 << 15


def graph_of(torch, fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        fn()
    return g


def in_turn(torch, graphs, reps):
    """Median milliseconds of every graph, replayed in turn `reps` times after one warm-up replay of each."""
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    ts = [[] for _ in graphs]
    for _ in range(reps):
        for g, t in zip(graphs, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return [sorted(t)[len(t) // 2] for t in ts]


class Circuit:
    def __init__(self, torch, pkg, ctx, k, n_sets, seed):
        self.pkg, self.ctx, self.k, self.n_sets, self.lay = pkg, ctx, k, n_sets, pkg.LAYOUT_PACKED
        self.n = pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(seed)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        pt = torch.from_numpy(rng.integers(0, 256, (self.n, 16), dtype=np.uint8)).cuda()
        self.kw = ctx.key_schedule_witness(key.reshape(1, 16), self.lay, want_rk=False)
        self.w = ctx.encrypt_witness(pt, key, layout=self.lay)
        self.st = [pkg.column_stride(self.lay, i) for i in range(3)]
        self.offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, [self.n], self.n).view(np.int64)).cuda()
        self.acc = ctx.multiplicity_accumulator(k, n_sets, self.lay)
        self.one = torch.empty((1, n_sets, pkg.TABLE_ROWS), dtype=torch.int32, device="cuda")
        self.rep = torch.empty(3, dtype=torch.int64, device="cuda")
        self.ks = pkg.api.KeySlab(*[t.data_ptr() for t in self.kw[:4]])

    def run(self, first, count):
        return self.pkg.Witness(*[t[first * s:(first + count) * s] for t, s in zip(self.w[:3], self.st)], None, None)

    def accumulate(self, chunk=0, runs=None):
        runs = [(0, self.n)] if runs is None else runs
        views = [(first, self.run(first, count)) for first, count in runs]

        def f():
            self.acc.reset()
            for first, view in views:
                self.acc.add(first, view, _chunk=chunk)
            self.acc.add_key(self.kw)
        return f

    def one_shot(self, form):
        lib, w = self.pkg.api.load_mult_library(), self.w

        def f():
            rc = lib.aesw_mult_count_device_form(self.ctx._h, self.k, self.n_sets, 1, self.offs.data_ptr(), self.lay, w.x.data_ptr(), w.y.data_ptr(),
                                                 w.z.data_ptr(), C.byref(self.ks), self.one.data_ptr(), self.rep.data_ptr(), self.ctx._stream(), form)
            if rc:
                raise RuntimeError("aesw_mult_count_device_form: %d" % rc)
        return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    alib = pkg.api.load_acc_library()
    res = {}
    big = Circuit(torch, pkg, ctx, 24, 4, 1)
    default = int(alib.aesw_acc_default_chunk(24, 4, 0, big.n))
    ts = in_turn(torch, [graph_of(torch, big.accumulate(chunk)) for chunk in CHUNKS], a.reps)
    res["chunk_k24_n4"] = {"blocks": big.n, "default_chunk": default, "us": {str(c or "default"): round(t * 1e3, 1) for c, t in zip(CHUNKS, ts)}}
    print("K=24 N=4, %d blocks, reset + add + add_key by chunk (default %d):" % (big.n, default), res["chunk_k24_n4"]["us"])
    for name, circ in (("one_k24_n4", big), ("one_k20_n4", Circuit(torch, pkg, ctx, 20, 4, 2))):
        fns = [circ.accumulate(), circ.one_shot(pkg.api.MULT_FORM_AUTO), circ.one_shot(pkg.api.MULT_FORM_PRIVATE)]
        fns[1]()
        torch.cuda.synchronize()
        want = circ.one.clone()
        fns[0]()
        torch.cuda.synchronize()
        assert torch.equal(circ.acc.histograms(), want[0]), "the accumulator and the one-shot count differ"
        ts = in_turn(torch, [graph_of(torch, f) for f in fns], a.reps)
        slab = circ.n * sum(circ.st)
        res[name] = {"blocks": circ.n, "slab_bytes": slab, "accumulator_us": round(ts[0] * 1e3, 1), "mult_auto_us": round(ts[1] * 1e3, 1),
                     "mult_private_us": round(ts[2] * 1e3, 1), "accumulator_GBps_of_slab_bytes": round(slab / (ts[0] * 1e-3) / 1e9, 1)}
        print(name, res[name])
    runs = [(first, min(STREAM_BLOCKS, big.n - first)) for first in range(0, big.n, STREAM_BLOCKS)]
    ts = in_turn(torch, [graph_of(torch, big.accumulate(runs=runs)), graph_of(torch, big.accumulate())], a.reps)
    res["stream_k24_n4"] = {"runs": len(runs), "run_blocks": STREAM_BLOCKS, "in_runs_us": round(ts[0] * 1e3, 1), "one_add_us": round(ts[1] * 1e3, 1)}
    print("stream shape:", res["stream_k24_n4"])
    ctx.close()
    line = json.dumps({"acc_bench": res})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
