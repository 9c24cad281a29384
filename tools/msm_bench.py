"""Timing of the commitments of libaesw_msm.so.

    python tools/msm_bench.py [--k 20] [--reps 11] [--build-only] [--out FILE]

One process; the basis is the generator at every row (the law is complete: adding P to P costs what any addition costs), the
scalars seeded canonical cells and seeded bytes; every figure the median of --reps graph replays taken in turn with the other
candidates of its group.
  * one byte column, one column of cells, eight columns of cells in one call against eight calls;
  * the slice count: one column of cells and one byte column with the slices forced to powers of two around the rule's;
  * every kernel alone: variants of the library built with -DAESW_MSM_PASSES=<one bit> (next to the product's, never loaded by
    the package) replayed over the workspace a whole call left behind;
  * the chunk length L: variants built with -DAESW_MSM_CHUNK=1024 and 8192, each under its own slice rule.
--build-only builds the variants and stops (no GPU needed).  One JSON line at the end (and into --out)."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.acc_bench import graph_of, in_turn  # noqa: E402  (the capture and the clock)

PASSES = {"digits": 1, "bucket": 2, "reduce": 4, "combine": 8}
CHUNKS = (1024, 8192)
FR, BYTES = 0, 1


def variants(build):
    """name -> path of every measurement variant, built where it is missing or stale"""
    out = {}
    for name, bit in PASSES.items():
        out["pass_" + name] = build.build_curve("msm", extra_flags=["-DAESW_MSM_PASSES=%d" % bit], out="libaesw_msm_pass_%s.so" % name)
    for chunk in CHUNKS:
        out["chunk_%d" % chunk] = build.build_curve("msm", extra_flags=["-DAESW_MSM_CHUNK=%d" % chunk], out="libaesw_msm_chunk_%d.so" % chunk)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import __graft_entry__ as ge
    build = ge._load_build()
    paths = variants(build)
    if a.build_only:
        print(json.dumps({name: str(p.name) for name, p in paths.items()}))
        return
    import numpy as np
    import torch
    ge.build()
    pkg = ge.load_package()
    api = pkg.api
    ctx = pkg.Context(0)
    lib = api.load_msm_library()
    k, n = a.k, 1 << a.k
    basis = torch.from_numpy(np.tile(api.g1_generator(), (n, 1))).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0x6d736d)
    cells = torch.randint(0, 256, (8, n, 32), dtype=torch.uint8, device="cuda", generator=gen)
    cells[:, :, 31] &= 0x1f  # below r, whatever the rest
    bytes_ = torch.randint(0, 256, (1, n), dtype=torch.uint8, device="cuda", generator=gen)
    out8 = torch.empty((8, 64), dtype=torch.uint8, device="cuda")

    def call(library, scalars, kind, slices, ws, out):
        def f():
            rc = library.aesw_msm_commit_device(ctx._h, k, scalars.shape[0], kind, slices, scalars.data_ptr(), basis.data_ptr(), out.data_ptr(), ws.data_ptr(), ctx._stream())
            assert rc == 0, api.STATUS.get(rc)
        return f

    def workspace(library, n_cols, kind, slices):
        return torch.empty(int(library.aesw_msm_workspace_bytes(k, n_cols, kind, slices)), dtype=torch.uint8, device="cuda")

    res = {"k": k, "reps": a.reps, "chunk": int(lib.aesw_msm_chunk_rows()), "slices_fr": int(lib.aesw_msm_slices(k, 1, FR, 0)), "slices_bytes": int(lib.aesw_msm_slices(k, 1, BYTES, 0))}
    ws1, wsb, ws8 = workspace(lib, 1, FR, 0), workspace(lib, 1, BYTES, 0), workspace(lib, 8, FR, 0)

    def eight_calls():
        for c in range(8):
            call(lib, cells[c:c + 1], FR, 0, ws1, out8[c:c + 1])()
    names = ("bytes_1", "fr_1", "fr_8_one_call", "fr_8_eight_calls")
    graphs = [graph_of(torch, f) for f in (call(lib, bytes_, BYTES, 0, wsb, out8[:1]), call(lib, cells[:1], FR, 0, ws1, out8[:1]), call(lib, cells, FR, 0, ws8, out8), eight_calls)]
    res["ms"] = dict(zip(names, in_turn(torch, graphs, a.reps)))
    print(res["ms"], flush=True)

    # the slice count
    for kind, scalars, label, counts in ((FR, cells[:1], "slices_ms_fr", (8, 16, 32, 64, 128)), (BYTES, bytes_, "slices_ms_bytes", (32, 64, 128, 256, 512, 1024))):
        wss = [workspace(lib, 1, kind, s) for s in counts]
        graphs = [graph_of(torch, call(lib, scalars, kind, s, w, out8[:1])) for s, w in zip(counts, wss)]
        res[label] = dict(zip(map(str, counts), in_turn(torch, graphs, a.reps)))
        print(label, res[label], flush=True)

    # every kernel alone, over the workspace of a whole call: one column of cells, and the bucket kernel of a byte column
    call(lib, cells[:1], FR, 0, ws1, out8[:1])()
    call(lib, bytes_, BYTES, 0, wsb, out8[:1])()
    torch.cuda.synchronize()
    alone = {name: api.load_msm_library(paths["pass_" + name]) for name in PASSES}
    graphs = [graph_of(torch, call(alone[name], cells[:1], FR, 0, ws1, out8[1:2])) for name in PASSES] + [graph_of(torch, call(alone["bucket"], bytes_, BYTES, 0, wsb, out8[1:2]))]
    res["kernel_ms_fr"] = dict(zip(list(PASSES) + ["bucket_bytes"], in_turn(torch, graphs, a.reps)))
    additions = 32 * n * 255 / 256  # a digit is zero once in 256
    res["bucket_additions_per_s"] = additions / (res["kernel_ms_fr"]["bucket"] * 1e-3)
    res["bucket_products_per_s"] = 11 * res["bucket_additions_per_s"]
    print(res["kernel_ms_fr"], "%.3g additions/s, %.3g products/s" % (res["bucket_additions_per_s"], res["bucket_products_per_s"]), flush=True)

    # the chunk length, each variant under its own rule
    libs = {res["chunk"]: lib}
    libs.update({chunk: api.load_msm_library(paths["chunk_%d" % chunk]) for chunk in CHUNKS})
    for kind, scalars, label in ((FR, cells[:1], "chunk_ms_fr"), (BYTES, bytes_, "chunk_ms_bytes")):
        order = sorted(libs)
        wss = [workspace(libs[c], 1, kind, 0) for c in order]
        graphs = [graph_of(torch, call(libs[c], scalars, kind, 0, w, out8[:1])) for c, w in zip(order, wss)]
        res[label] = {"%d (%d slices)" % (c, libs[c].aesw_msm_slices(k, 1, kind, 0)): t for c, t in zip(order, in_turn(torch, graphs, a.reps))}
        print(label, res[label], flush=True)

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
