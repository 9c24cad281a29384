"""Timing of the compression under theta (libaesw_theta.so).

    python tools/theta_bench.py [--reps 21] [--k 20] [--sets 4] [--out FILE]

One process, one circuit at K / N filled to its capacity; every figure the median of --reps graph replays taken in turn with the
other candidates of its group.
  * columns: aesw_theta_columns_device over the 5 N arguments of A', of the input indices and of the table column in row order
    (NULL), next to the 5 N aesw_perm_gather_fr_device calls over A' that one call replaces;
  * inputs: aesw_theta_inputs_device from PACKED and from DENSE slabs next to a fill_ of the bytes it writes;
  * compress: aesw_theta_compress_table_device.
One JSON line at the end (and into --out)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.acc_bench import graph_of, in_turn  # noqa: E402  (the capture and the clock)

TABLE_OF_TAG = (0, 2, 1, 1, 1)


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
    lib = pkg.api.load_theta_library()
    k, n_sets, u = arg.k, arg.sets, 1 << arg.k
    n_args, n = 5 * n_sets, pkg.block_capacity(k, n_sets)
    rng = np.random.default_rng(k)
    key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    slabs = {l: (ctx.encrypt_witness(pt, key, layout=l), ctx.key_schedule_witness(key.reshape(1, 16), l, want_rk=False)) for l in (pkg.LAYOUT_PACKED, pkg.LAYOUT_DENSE)}
    w, kw = slabs[pkg.LAYOUT_PACKED]
    mult, rep = ctx.lookup_multiplicities(k, n_sets, w, kw, [n])
    assert rep["misses"] == 0
    a, _s, _ = ctx.permuted_columns(k, n_sets, mult)
    index, irep = ctx.lookup_inputs(k, n_sets, w, kw)
    assert irep == rep
    d_theta = torch.from_numpy(pkg.api.fr_cell(int.from_bytes(rng.bytes(40), "little"))).cuda()
    table, _ = ctx.compress_table(d_theta)
    out = torch.empty((n_sets, 5, u, 32), dtype=torch.uint8, device="cuda")

    def twenty():
        for st in range(n_sets):
            for t in range(5):
                ctx.gather_fr(a[st, t], table[TABLE_OF_TAG[t]], out=out[st, t])

    graphs = [graph_of(torch, lambda: ctx.argument_columns(a, table, k, n_sets, out=out)), graph_of(torch, lambda: ctx.argument_columns(index, table, k, n_sets, out=out)),
              graph_of(torch, lambda: ctx.argument_columns(None, table, k, n_sets, out=out)), graph_of(torch, twenty)]
    ts = in_turn(torch, graphs, arg.reps)
    written = out.numel()
    res = {"k": k, "n_sets": n_sets, "blocks": n, "arguments": n_args, "column_bytes": written,
           "columns_us": {name: round(t * 1e3, 1) for name, t in zip(("a_prime", "inputs", "table_row_order", "per_argument_gathers"), ts)},
           "columns_tb_per_s": round(written / ts[0] / 1e9, 2), "fused_over_gathers": round(ts[0] / ts[3], 4)}
    print("K=%d N=%d, %d blocks, %d arguments:" % (k, n_sets, n, n_args), res)

    d_in = torch.empty((n_sets, 5, u), dtype=torch.int32, device="cuda")
    rep_t = torch.empty(3, dtype=torch.int64, device="cuda")

    def inputs(layout):
        wl, kl = slabs[layout]
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in kl[:4]])

        def f():
            rc = lib.aesw_theta_inputs_device(ctx._h, k, n_sets, n, layout, wl.x.data_ptr(), wl.y.data_ptr(), wl.z.data_ptr(), C.byref(ks), d_in.data_ptr(),
                                              rep_t.data_ptr(), ctx._stream())
            assert rc == 0, ctx._lib.aesw_last_error(ctx._h)
        return f

    def captured(f):  # the workspace belongs to (context, stream): prepared for the stream that captures
        side = torch.cuda.Stream()
        assert lib.aesw_theta_prepare(ctx._h, k, n_sets, C.c_void_p(side.cuda_stream)) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            f()
        return g

    crep = torch.empty(2, dtype=torch.int64, device="cuda")
    graphs = [captured(inputs(pkg.LAYOUT_PACKED)), captured(inputs(pkg.LAYOUT_DENSE)), graph_of(torch, lambda: d_in.fill_(66560)),
              graph_of(torch, lambda: lib.aesw_theta_compress_table_device(ctx._h, d_theta.data_ptr(), table.data_ptr(), crep.data_ptr(), ctx._stream()))]
    tp, td, tf, tc = in_turn(torch, graphs, arg.reps)
    in_bytes = d_in.numel() * 4
    res.update(inputs_bytes=in_bytes, inputs_us={"packed": round(tp * 1e3, 1), "dense": round(td * 1e3, 1)}, fill_us=round(tf * 1e3, 1),
               inputs_tb_per_s=round(in_bytes / tp / 1e9, 2), fill_tb_per_s=round(in_bytes / tf / 1e9, 2), compress_us=round(tc * 1e3, 1))
    print("inputs against a fill_, and the compress call:", {key_: res[key_] for key_ in ("inputs_us", "fill_us", "compress_us")})
    ctx.close()
    line = json.dumps({"theta_bench": res})
    print(line)
    if arg.out:
        Path(arg.out).parent.mkdir(parents=True, exist_ok=True)
        Path(arg.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
