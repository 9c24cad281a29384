"""Timing of the lookup multiplicities (aesw_mult_count_device, libaesw_mult.so): both forms against the one-launch many-circuit
checker over the same batch.

    python tools/mult_bench.py [--reps 5] [--max-out-gb 24] [--out FILE]

One process; per shape the three launches -- DIRECT, PRIVATE, aesw_circ_check_witness_device -- run in turn over the same PACKED
buffers, median of --reps.  Shapes: K = 20 / N = 4 circuits filled to 2^20 blocks, K = 12 / N = 1 (one block per circuit) with the
same number of blocks, and both at 2^16 blocks.  A shape whose histograms ([C][N][66561] uint32) need more than --max-out-gb is
not run and says so: 2^20 one-block circuits need 279 GB of them.

Printed per shape and form: microseconds, the bytes a linear read of the slabs moves (every block and key slab once), the bytes
the form reads (PRIVATE: twice, its two workgroups per circuit and set both walk the blocks), the bytes it writes (DIRECT: the
zeroing pass, then 4 bytes per lookup as atomics), and the read rate the time amounts to against the linear bytes.  One JSON
line at the end (and into --out)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FORMS = {"direct": 1, "private": 2}


def in_turn(torch, fns, reps):
    """Median milliseconds of every fn, run in turn `reps` times after one warm-up of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return [sorted(t)[len(t) // 2] for t in ts]


def shape(torch, pkg, ctx, k, n_sets, blocks, reps, max_out_bytes, seed):
    lay = pkg.LAYOUT_PACKED
    cap = pkg.block_capacity(k, n_sets)
    nc = max(1, blocks // cap)
    n = nc * cap
    out_bytes = nc * n_sets * pkg.TABLE_ROWS * 4
    res = {"k": k, "n_sets": n_sets, "circuits": nc, "blocks": n, "histogram_bytes": out_bytes}
    if out_bytes > max_out_bytes:
        res["not_measured"] = "the histograms need %.1f GB" % (out_bytes / 1e9)
        return res
    rng = np.random.default_rng(seed)
    keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    kw = ctx.key_schedule_witness(keys, lay, want_rk=False)
    w = ctx.encrypt_witness(pt, torch.repeat_interleave(keys, cap, dim=0), layout=lay, want_ct=True)
    offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, [cap] * nc, n).view(np.int64)).cuda()
    mult = torch.empty((nc, n_sets, pkg.TABLE_ROWS), dtype=torch.int32, device="cuda")
    rep3, rep8 = torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(8, dtype=torch.int64, device="cuda")
    ks = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
    mlib, clib = pkg.api.load_mult_library(), pkg.api.load_circ_library()
    margs = (ctx._h, k, n_sets, nc, offs.data_ptr(), lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(), C.byref(ks), mult.data_ptr(),
             rep3.data_ptr(), ctx._stream())
    cargs = (ctx._h, k, n_sets, nc, offs.data_ptr(), n, pt.data_ptr(), keys.data_ptr(), lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(),
             w.ct.data_ptr(), C.byref(ks), rep8.data_ptr(), ctx._stream())

    def count(form):
        def f():
            rc = mlib.aesw_mult_count_device_form(*margs, form)
            if rc:
                raise RuntimeError("aesw_mult_count_device_form: %d" % rc)
        return f

    def check():
        rc = clib.aesw_circ_check_witness_device(*cargs)
        if rc:
            raise RuntimeError("aesw_circ_check_witness_device: %d" % rc)

    # the two forms give the same bytes before either is timed
    sums = []
    for form in FORMS.values():
        mult.fill_(-1)
        count(form)()
        torch.cuda.synchronize()
        sums.append((int(mult.sum(dtype=torch.int64)), mult.clone() if out_bytes <= 1 << 30 else None, rep3.cpu().tolist()))
    lookups = 400 * nc + 1056 * n
    assert sums[0][0] == sums[1][0] == lookups and sums[0][2] == sums[1][2] == [lookups, 0, -1], (sums[0][0], sums[1][0], lookups, sums[0][2])
    if sums[0][1] is not None:
        assert torch.equal(sums[0][1], sums[1][1])
    sums = None
    t = in_turn(torch, [count(FORMS["direct"]), count(FORMS["private"]), check], reps)
    assert rep8.cpu().tolist()[:6] == [n, nc, 0, 0, 0, 0]
    st = [pkg.column_stride(lay, i) for i in range(3)]
    kst = [pkg.key_column_stride(lay, i) for i in range(3)]
    linear = n * sum(st) + nc * sum(kst)
    res.update(default_form=[name for name, f in FORMS.items() if f == mlib.aesw_mult_default_form(k, n_sets, nc)][0], linear_read_bytes=linear,
               circ_check_us=round(t[2] * 1e3, 1))
    for name, ms, read, written in (("direct", t[0], linear, out_bytes + 4 * lookups), ("private", t[1], 2 * n * sum(st) + nc * sum(kst), out_bytes)):
        res[name] = {"us": round(ms * 1e3, 1), "bytes_read": read, "bytes_written": written,
                     "linear_read_GBps": round(linear / (ms * 1e-3) / 1e9, 1), "written_GBps": round(written / (ms * 1e-3) / 1e9, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-out-gb", type=float, default=24.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    res = {}
    for name, (k, n_sets, blocks) in {"k20_n4_2p20": (20, 4, 1 << 20), "k12_n1_2p20": (12, 1, 1 << 20), "k20_n4_2p16": (20, 4, 1 << 16),
                                      "k12_n1_2p16": (12, 1, 1 << 16)}.items():
        r = res[name] = shape(torch, pkg, ctx, k, n_sets, blocks, a.reps, int(a.max_out_gb * 1e9), seed=len(res))
        if "not_measured" in r:
            print("%-12s C=%d: not measured, %s" % (name, r["circuits"], r["not_measured"]))
            continue
        print("%-12s C=%d, %d blocks, histograms %.1f MB, default %s; circ check %.1f us" % (
            name, r["circuits"], r["blocks"], r["histogram_bytes"] / 1e6, r["default_form"], r["circ_check_us"]))
        for form in FORMS:
            f = r[form]
            print("  %-8s %10.1f us   read %d B (linear %d B: %.1f GB/s)   written %d B (%.1f GB/s)" % (
                form, f["us"], f["bytes_read"], r["linear_read_bytes"], f["linear_read_GBps"], f["bytes_written"], f["written_GBps"]))
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps({"mult_bench": res})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
