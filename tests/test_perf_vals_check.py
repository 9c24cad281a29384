"""Timing condition of the values checker (`pytest -m perf` on a GPU box; the `perf` marker only).  No absolute time is fixed:
aesw_vals_check_device is compared with the existing PACKED aesw_check_witness_device over the same 2^20 blocks with per-block
keys, in one process, alternating, median of five (the method of tests/test_perf_circ_check.py).  The values check reads about
half the bytes and walks 1 056 rows where the PACKED check walks 1 360 rows and 1 952 edges, so the condition is
t_values < t_packed; the 1-3 % replay drift of DESIGN 5 cannot flip a comparison that work counts put near one half.  Every
figure is printed before it is asserted (run with -s).  Figures belong in DESIGN 4.14 and profiles/vals/README.md; none were recorded when this
was written (no GPU was available)."""
import ctypes as C

import numpy as np
import pytest

from test_perf_circ_check import _alternate, gpu  # noqa: F401  (gpu: the module's fixture, skips without a GPU)

pytestmark = pytest.mark.perf


def _pair(torch, pkg, ctx, n, pbk, seed):
    rng = np.random.default_rng(seed)
    pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
    keys = torch.from_numpy(rng.integers(0, 256, (n, 16) if pbk else 16, dtype=np.uint8)).cuda()
    v = ctx.encrypt_witness(pt, keys, layout=pkg.LAYOUT_VALUES, want_ct=True, key_slab=True)
    p = ctx.encrypt_witness(pt, keys, layout=pkg.LAYOUT_PACKED, want_ct=True, key_slab=True)
    rep_v, rep_p = torch.zeros(7, dtype=torch.int64, device="cuda"), torch.zeros(7, dtype=torch.int64, device="cuda")
    ks_v, ks_p = pkg.api.KeySlab(*[t.data_ptr() for t in v.key[:4]]), pkg.api.KeySlab(*[t.data_ptr() for t in p.key[:4]])
    vals, lib = pkg.api.load_vals_library(), ctx._lib

    def f_values():
        assert vals.aesw_vals_check_device(ctx._h, pt.data_ptr(), keys.data_ptr(), 1 if pbk else 0, n, v.y.data_ptr(), v.z.data_ptr(), v.ct.data_ptr(),
                                           C.byref(ks_v), rep_v.data_ptr(), ctx._stream()) == 0

    def f_packed():
        assert lib.aesw_check_witness_device(ctx._h, pt.data_ptr(), keys.data_ptr(), 1 if pbk else 0, n, pkg.LAYOUT_PACKED, p.x.data_ptr(), p.y.data_ptr(),
                                             p.z.data_ptr(), p.ct.data_ptr(), C.byref(ks_p), rep_p.data_ptr(), ctx._stream()) == 0
    f_values.keep = (v, p, pt, keys, ks_v, ks_p)
    return f_values, f_packed, rep_v, rep_p


def _run(torch, pkg, ctx, n, pbk, seed):
    f_values, f_packed, rep_v, rep_p = _pair(torch, pkg, ctx, n, pbk, seed)
    t_v, t_p = _alternate(torch, f_values, f_packed)
    torch.cuda.synchronize()
    clean = [n, n if pbk else 1, 0, 0, 0, 0, -1]
    assert rep_v.cpu().tolist() == clean and rep_p.cpu().tolist() == clean
    print("\n%d blocks, %s: values check %.3f ms (%.2e blocks/s), packed check %.3f ms (%.2e blocks/s), ratio %.3f"
          % (n, "per-block keys" if pbk else "shared key", t_v, n / t_v * 1e3, t_p, n / t_p * 1e3, t_v / t_p))
    return t_v, t_p


def test_the_values_check_is_faster_than_the_packed_check_at_the_headline_size(gpu, pkg, ctx):
    t_v, t_p = _run(gpu, pkg, ctx, 1 << 20, True, 1)
    assert t_v < t_p, (t_v, t_p)


def test_the_same_comparison_for_a_shared_key_is_recorded(gpu, pkg, ctx):
    """2^16 blocks with a shared key: printed and recorded, no condition attached."""
    t_v, t_p = _run(gpu, pkg, ctx, 1 << 16, False, 2)
    assert t_v > 0 and t_p > 0
