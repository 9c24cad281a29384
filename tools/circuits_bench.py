"""Many circuits per launch against what they replace (kernel times from HIP events, median of --reps after a warm-up).

    python tools/circuits_bench.py [--reps 20] [--out FILE]

assemble  Fr advice.  K = 20, N = 5, C = 4 full circuits: one circuit_assemble_kernel launch against four
          aesw_assemble_advice_device calls.  K = 14, N = 1, C = 4 096 full circuits (10 blocks each): one launch against a
          loop of 4 096 calls on one stream.  Both compared byte for byte once.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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
    asm = {}
    for name, (k, n_sets, nc) in {"k20_n5_c4": (20, 5, 4), "k14_n1_c4096": (14, 1, 4096)}.items():
        cap = pkg.block_capacity(k, n_sets)
        counts = [cap] * nc
        m = cap * nc
        keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
        kw = ctx.key_schedule_witness(keys, lay, want_rk=False)
        w = ctx.encrypt_witness(torch.from_numpy(rng.integers(0, 256, (m, 16), dtype=np.uint8)).cuda(),
                                torch.repeat_interleave(keys, cap, dim=0), layout=lay)
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
        del out, ref, w, kw, args
        torch.cuda.empty_cache()
    res["assemble_fr"] = asm
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
