"""Many circuits per launch against what they replace (kernel times from HIP events, median of --reps after a warm-up).

    python tools/circuits_bench.py [--reps 20] [--check] [--out FILE]

assemble  Fr advice.  K = 20, N = 5, C = 4 full circuits: one circuit_assemble_kernel launch against four
          aesw_assemble_advice_device calls.  K = 14, N = 1, C = 4 096 full circuits (10 blocks each): one launch against a
          loop of 4 096 calls on one stream.  Both compared byte for byte once.
check     (--check) the batches the assemble part made, certified by the one-launch many-circuit checker
          (aesw_circ_check_witness_device), and that launch timed against C one-circuit aesw_check_witness_device calls on one
          stream over the same buffers (alternating, median).  K = 20, N = 5 also with C = 256 against the per-block-key check
          of the same number of blocks.
Run under `rocprofv3 --kernel-trace --stats` for per-kernel times of the same calls."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(torch, fn, reps):
    """Median milliseconds of fn() between two events on the current stream, and all samples."""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], ts


def alternating(torch, f, g, reps):
    """Median milliseconds of f() and g(), run in turn."""
    f(), g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    return sorted(tf)[len(tf) // 2], sorted(tg)[len(tg) // 2]


def check_part(torch, pkg, ctx, k, n_sets, nc, cap, keys, pt, w, kw, offs, reps):
    """The batch certified in one launch, and that launch against nc one-circuit check calls (prepared arguments: launches, not Python)."""
    lay, m = pkg.LAYOUT_PACKED, cap * nc
    lib = pkg.api.load_circ_library()
    rep = torch.empty(8, dtype=torch.int64, device="cuda")
    reps7 = torch.empty((nc, 7), dtype=torch.int64, device="cuda")
    slab = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
    stream = ctx._stream()
    one_args = (ctx._h, k, n_sets, nc, offs.data_ptr(), m, pt.data_ptr(), keys.data_ptr(), lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(),
                w.ct.data_ptr(), C.byref(slab), rep.data_ptr(), stream)
    st = [pkg.column_stride(lay, i) for i in range(3)]
    ks = [96] + [pkg.key_column_stride(lay, i) for i in range(3)]
    kz = torch.zeros((nc, 208), dtype=torch.uint8, device="cuda")  # packed kz slabs are 200 B apart: copies on 16-byte boundaries
    kz[:, :ks[3]] = kw.kz.view(nc, ks[3])
    slabs = [pkg.api.KeySlab(kw.w.data_ptr() + c * ks[0], kw.kx.data_ptr() + c * ks[1], kw.ky.data_ptr() + c * ks[2], kz.data_ptr() + c * 208)
             for c in range(nc)]
    args = [(ctx._h, pt.data_ptr() + 16 * c * cap, keys.data_ptr() + 16 * c, 0, cap, lay, w.x.data_ptr() + c * cap * st[0],
             w.y.data_ptr() + c * cap * st[1], w.z.data_ptr() + c * cap * st[2], w.ct.data_ptr() + 16 * c * cap, C.byref(slabs[c]),
             reps7[c].data_ptr(), stream) for c in range(nc)]

    def one():
        rc = lib.aesw_circ_check_witness_device(*one_args)
        if rc:
            raise RuntimeError("aesw_circ_check_witness_device: %d" % rc)

    def loop():
        for a_ in args:
            rc = ctx._lib.aesw_check_witness_device(*a_)
            if rc:
                raise RuntimeError("aesw_check_witness_device: %d" % rc)

    t_one, t_loop = alternating(torch, one, loop, reps)
    r = pkg.api.circ_report_dict(rep)
    singles_ok = not bool(reps7[:, 2:6].any().item())
    return {"circuits": nc, "blocks": m, "one_launch_us": round(t_one * 1e3, 1), "single_calls_us": round(t_loop * 1e3, 1),
            "speedup": round(t_loop / t_one, 2), "certified": bool(r["satisfied"] and r["blocks"] == m and r["keys"] == nc and singles_ok)}


def check_vs_per_block_keys(torch, pkg, ctx, k, n_sets, nc, rng, reps):
    """About 2^20 blocks: the many-circuit check against the per-block-key check of the same number of blocks."""
    lay, cap = pkg.LAYOUT_PACKED, pkg.block_capacity(k, n_sets)
    m = cap * nc
    keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (m, 16), dtype=np.uint8)).cuda()
    bkeys = torch.repeat_interleave(keys, cap, dim=0)
    kw = ctx.key_schedule_witness(keys, lay, want_rk=False)
    w = ctx.encrypt_witness(pt, bkeys, layout=lay, want_ct=True, key_slab=True)  # w.key: one key slab per block, for the per-block-key form
    offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, [cap] * nc, m).view(np.int64)).cuda()
    rep, rep7 = torch.empty(8, dtype=torch.int64, device="cuda"), torch.empty(7, dtype=torch.int64, device="cuda")
    slab, bslab = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]]), pkg.api.KeySlab(*[t.data_ptr() for t in w.key[:4]])
    stream = ctx._stream()
    lib = pkg.api.load_circ_library()
    a1 = (ctx._h, k, n_sets, nc, offs.data_ptr(), m, pt.data_ptr(), keys.data_ptr(), lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(),
          w.ct.data_ptr(), C.byref(slab), rep.data_ptr(), stream)
    a2 = (ctx._h, pt.data_ptr(), bkeys.data_ptr(), 1, m, lay, w.x.data_ptr(), w.y.data_ptr(), w.z.data_ptr(), w.ct.data_ptr(), C.byref(bslab),
          rep7.data_ptr(), stream)

    def one():
        if lib.aesw_circ_check_witness_device(*a1):
            raise RuntimeError("aesw_circ_check_witness_device")

    def pbk():
        if ctx._lib.aesw_check_witness_device(*a2):
            raise RuntimeError("aesw_check_witness_device")

    t_one, t_pbk = alternating(torch, one, pbk, reps)
    r = pkg.api.circ_report_dict(rep)
    return {"circuits": nc, "blocks": m, "many_circuit_us": round(t_one * 1e3, 1), "per_block_key_us": round(t_pbk * 1e3, 1),
            "ratio": round(t_one / t_pbk, 3), "certified": bool(r["satisfied"] and r["blocks"] == m and r["keys"] == nc and not rep7[2:6].any().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check", action="store_true", help="certify every batch with the one-launch checker and time it against one check call per circuit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    lay = pkg.LAYOUT_PACKED
    ctx = pkg.Context(0)
    rng = np.random.default_rng(0xC1C)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}

    # ---- assemble (Fr)
    asm, chk = {}, {}
    for name, (k, n_sets, nc) in {"k20_n5_c4": (20, 5, 4), "k14_n1_c4096": (14, 1, 4096)}.items():
        cap = pkg.block_capacity(k, n_sets)
        counts = [cap] * nc
        m = cap * nc
        keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
        kw = ctx.key_schedule_witness(keys, lay, want_rk=False)
        pt = torch.from_numpy(rng.integers(0, 256, (m, 16), dtype=np.uint8)).cuda()
        w = ctx.encrypt_witness(pt, torch.repeat_interleave(keys, cap, dim=0), layout=lay, want_ct=a.check)
        ncol = 3 * n_sets + 1
        out = torch.empty((nc, ncol, 1 << k, 32), dtype=torch.uint8, device="cuda")
        ref = torch.empty_like(out)
        offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, counts, m).view(np.int64)).cuda()
        st = [pkg.column_stride(lay, i) for i in range(3)]
        ks = [96] + [pkg.key_column_stride(lay, i) for i in range(3)]
        singles = [(pkg.Witness(*[w[i][c * cap * st[i]:(c + 1) * cap * st[i]] for i in range(3)], None, None),
                    pkg.KeyWitness(*[kw[i][c * ks[i]:(c + 1) * ks[i]] for i in range(4)], None)) for c in range(nc)]

        def one():
            ctx.assemble_advice_circuits(k, n_sets, w, kw, counts, as_fr=True, out=out, _offsets=offs)

        # the loop calls the C ABI directly with prepared arguments, so that what is timed is launches, not Python
        stream = ctx._stream()
        args = [(ctx._h, k, n_sets, cap, lay, w1.x.data_ptr(), w1.y.data_ptr(), w1.z.data_ptr(),
                 C.byref(pkg.api.KeySlab(*[t.data_ptr() for t in k1[:4]])), 1, ref[c].data_ptr(), stream) for c, (w1, k1) in enumerate(singles)]

        def loop():
            for a_ in args:
                rc = ctx._lib.aesw_assemble_advice_device(*a_)
                if rc:
                    raise RuntimeError("aesw_assemble_advice_device: %d" % rc)

        t_one, s_one = timed(torch, one, a.reps)
        t_loop, s_loop = timed(torch, loop, max(3, a.reps // 4))
        nbytes = out.numel()
        asm[name] = {"circuits": nc, "blocks_per_circuit": cap, "bytes": nbytes,
                     "one_launch_us": round(t_one * 1e3, 1), "one_launch_TBps": round(nbytes / (t_one * 1e-3) / 1e12, 3),
                     "single_calls_us": round(t_loop * 1e3, 1), "single_calls_TBps": round(nbytes / (t_loop * 1e-3) / 1e12, 3),
                     "speedup": round(t_loop / t_one, 2), "identical": bool(torch.equal(out, ref))}
        if a.check:
            chk[name] = check_part(torch, pkg, ctx, k, n_sets, nc, cap, keys, pt, w, kw, offs, max(5, a.reps // 4))
        del out, ref, w, kw, args
        torch.cuda.empty_cache()
    res["assemble_fr"] = asm
    if a.check:
        chk["k20_n5_c256_vs_per_block_keys"] = check_vs_per_block_keys(torch, pkg, ctx, 20, 5, 256, rng, max(5, a.reps // 4))
        res["check"] = chk
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
