"""Timing of the multiplicity accumulator over a VALUES witness (libaesw_vacc.so) against the PACKED accumulator of
libaesw_acc.so (4.16).

    python tools/vacc_bench.py [--reps 21] [--waves16] [--out FILE]

One process, one circuit at K = 24 / N = 4 filled to its capacity, the same key and plaintexts as a VALUES and as a PACKED witness;
every figure the median of --reps graph replays taken in turn with the other candidates of its group.
  * VALUES against PACKED: reset + one add + add_key, both at the default chunk;
  * chunk size: the VALUES add with the blocks per pair of workgroups forced to 64, 128, 256, 512, 1 024, 2 048 and left to the
    default rule;
  * --waves16: the wave-count A/B.  A variant of the library built with -DAESW_VACC_WAVES=16 (next to the product's, never
    loaded by the package) is timed in turn with the product's 8 waves.  Its resource row is printed first: the variant is a
    candidate only if it keeps within 128 VGPRs without scratch.
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

CHUNKS = (64, 128, 256, 512, 1024, 2048, 0)
W16 = "libaesw_vacc_w16.so"


class Circuit:
    def __init__(self, torch, pkg, ctx, k, n_sets, seed):
        self.pkg, self.ctx, self.k, self.n_sets = pkg, ctx, k, n_sets
        self.n = pkg.block_capacity(k, n_sets)
        rng = np.random.default_rng(seed)
        key = torch.from_numpy(rng.integers(0, 256, 16, dtype=np.uint8)).cuda()
        self.pt = torch.from_numpy(rng.integers(0, 256, (self.n, 16), dtype=np.uint8)).cuda()
        self.kw = ctx.key_schedule_witness(key.reshape(1, 16), pkg.LAYOUT_PACKED, want_rk=False)
        self.packed = ctx.encrypt_witness(self.pt, key, layout=pkg.LAYOUT_PACKED)
        self.vals = ctx.encrypt_witness(self.pt, key, layout=pkg.LAYOUT_VALUES)
        self.acc = ctx.multiplicity_accumulator(k, n_sets)
        self.ks = pkg.api.KeySlab(self.kw[0].data_ptr(), None, None, self.kw[3].data_ptr())

    def from_packed(self):
        def f():
            self.acc.reset().add(0, self.packed).add_key(self.kw)
        return f

    def from_values(self, chunk=0, lib=None):
        """reset + add_values + add_key; lib: another build of libaesw_vacc.so to take the add from"""
        def f():
            self.acc.reset()
            if lib is None:
                self.acc.add_values(0, self.pt, self.vals, self.kw, _chunk=chunk)
            else:
                rc = lib.aesw_vacc_add_device_chunk(self.ctx._h, self.k, self.n_sets, 0, self.n, self.pt.data_ptr(), self.vals.y.data_ptr(),
                                                    self.vals.z.data_ptr(), C.byref(self.ks), self.acc._mult.data_ptr(), self.acc._rep.data_ptr(),
                                                    self.ctx._stream(), chunk)
                if rc:
                    raise RuntimeError("aesw_vacc_add_device_chunk: %d" % rc)
            self.acc.add_key(self.kw)
        return f

    def histograms_of(self, torch, f):
        f()
        torch.cuda.synchronize()
        return self.acc.histograms().clone(), self.acc.report()


def resources(pkg, lib_path):
    """the kernel's row of the resource table (tests/check_library.py), or None without the LLVM tools"""
    sys.path.insert(0, str(ROOT / "tests"))
    import tempfile
    try:
        from isa_extract import extract
        meta = next(iter(extract(lib_path, Path(tempfile.mkdtemp()))["meta"].values()))
        return {"vgpr": meta[".vgpr_count"], "scratch_bytes": meta[".private_segment_fixed_size"], "vgpr_spills": meta.get(".vgpr_spill_count", 0),
                "static_lds": meta[".group_segment_fixed_size"]}
    except Exception as e:  # a measurement aid, not a check
        return {"error": str(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--waves16", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    pkg = ge.load_package()
    ctx = pkg.Context(0)
    vlib = pkg.api.load_vacc_library()
    assert vlib.aesw_vacc_prepare(ctx._h) == 0
    res = {}
    big = Circuit(torch, pkg, ctx, 24, 4, 1)
    want, want_rep = big.histograms_of(torch, big.from_packed())
    got, got_rep = big.histograms_of(torch, big.from_values())
    assert torch.equal(got, want) and got_rep == want_rep, "the VALUES and the PACKED accumulation differ"
    default = int(vlib.aesw_vacc_default_chunk(24, 4, 0, big.n))
    ts = in_turn(torch, [graph_of(torch, big.from_values()), graph_of(torch, big.from_packed())], a.reps)
    bytes_v, bytes_p = big.n * 1072, big.n * sum(pkg.column_stride(pkg.LAYOUT_PACKED, i) for i in range(3))
    res["values_vs_packed_k24_n4"] = {"blocks": big.n, "default_chunk": default, "values_us": round(ts[0] * 1e3, 1), "packed_us": round(ts[1] * 1e3, 1),
                                      "ratio": round(ts[0] / ts[1], 3), "values_bytes": bytes_v, "packed_bytes": bytes_p,
                                      "values_blocks_per_s": round(big.n / (ts[0] * 1e-3))}
    print("K=24 N=4, %d blocks, reset + add + add_key:" % big.n, res["values_vs_packed_k24_n4"])
    ts = in_turn(torch, [graph_of(torch, big.from_values(chunk)) for chunk in CHUNKS], a.reps)
    res["chunk_k24_n4"] = {"default_chunk": default, "us": {str(c or "default"): round(t * 1e3, 1) for c, t in zip(CHUNKS, ts)}}
    print("VALUES by chunk (default %d):" % default, res["chunk_k24_n4"]["us"])
    if a.waves16:
        path = ge._load_build().build_satellite("vacc", extra_flags=["-DAESW_VACC_WAVES=16"], out=W16)
        row = resources(pkg, path)
        w16 = pkg.api.load_vacc_library(path)  # an explicit path: loaded anew, never cached
        assert w16.aesw_vacc_prepare(ctx._h) == 0
        got, got_rep = big.histograms_of(torch, big.from_values(lib=w16))
        assert torch.equal(got, want) and got_rep == want_rep, "the 16-wave build counts differently"
        ts = in_turn(torch, [graph_of(torch, big.from_values()), graph_of(torch, big.from_values(lib=w16))], a.reps)
        res["waves_k24_n4"] = {"waves8_us": round(ts[0] * 1e3, 1), "waves16_us": round(ts[1] * 1e3, 1), "waves8": resources(pkg, pkg.api.VACC_LIB_PATH),
                               "waves16": row}
        print("8 against 16 waves:", res["waves_k24_n4"])
    ctx.close()
    line = json.dumps({"vacc_bench": res})
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
