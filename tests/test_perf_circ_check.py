"""Timing conditions of the many-circuit checker (`pytest -m perf` on a GPU box; the `perf` marker only, so a noisy lease cannot
redden the parity suite).  No absolute time is fixed: both tests compare two forms in the same process over the same buffers,
alternating, median of five repeats each.  Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.perf


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("timing conditions need a GPU")
    return torch


def _ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(torch, f, g, reps=5):
    """Medians of f and g, run in turn `reps` times after one warm-up of each."""
    f(), g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(_ms(torch, f))
        tg.append(_ms(torch, g))
    return sorted(tf)[reps // 2], sorted(tg)[reps // 2]


def _batch(torch, pkg, ctx, k, n_sets, nc, seed):
    cap = pkg.block_capacity(k, n_sets)
    rng = np.random.default_rng(seed)
    keys = torch.from_numpy(rng.integers(0, 256, (nc, 16), dtype=np.uint8)).cuda()
    pt = torch.from_numpy(rng.integers(0, 256, (cap * nc, 16), dtype=np.uint8)).cuda()
    kw = ctx.key_schedule_witness(keys, pkg.LAYOUT_PACKED, want_rk=False)
    w = ctx.encrypt_witness(pt, torch.repeat_interleave(keys, cap, dim=0), layout=pkg.LAYOUT_PACKED, want_ct=True)
    offs = torch.from_numpy(pkg.circuit_offsets(k, n_sets, [cap] * nc, cap * nc).view(np.int64)).cuda()
    return cap, keys, pt, kw, w, offs


def _one_launch(pkg, ctx, k, n_sets, nc, n, keys, pt, kw, w, offs, rep):
    lib = pkg.api.load_circ_library()
    ks = pkg.api.KeySlab(*[t.data_ptr() for t in kw[:4]])
    args = (ctx._h, k, n_sets, nc, offs.data_ptr(), n, pt.data_ptr(), keys.data_ptr(), pkg.LAYOUT_PACKED, w.x.data_ptr(), w.y.data_ptr(),
            w.z.data_ptr(), w.ct.data_ptr(), C.byref(ks), rep.data_ptr(), ctx._stream())

    def f():
        rc = lib.aesw_circ_check_witness_device(*args)
        assert rc == 0, rc
    f.keep = ks
    return f


def test_one_launch_beats_a_check_call_per_circuit(gpu, pkg):
    """K = 14, N = 1, C = 4 096 full circuits of ten blocks: one launch against 4 096 one-circuit shared-key check calls on one
    stream (the C ABI with prepared arguments: launches are timed, not Python).  Only key slabs of even circuits are legal
    inputs of the one-circuit call in the packed layout (kz + 200 c), so the loop runs over aligned COPIES of every slab."""
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets, nc = 14, 1, 4096
        cap, keys, pt, kw, w, offs = _batch(torch, pkg, ctx, k, n_sets, nc, 1)
        n, lay = cap * nc, pkg.LAYOUT_PACKED
        rep = torch.empty(8, dtype=torch.int64, device="cuda")
        reps = torch.empty((nc, 7), dtype=torch.int64, device="cuda")
        one = _one_launch(pkg, ctx, k, n_sets, nc, n, keys, pt, kw, w, offs, rep)
        st = [pkg.column_stride(lay, i) for i in range(3)]
        kz = torch.zeros((nc, 208), dtype=torch.uint8, device="cuda")  # every slab of kz on a 16-byte boundary
        kz[:, :200] = kw.kz.view(nc, 200)
        kst = [96, pkg.key_column_stride(lay, 0), pkg.key_column_stride(lay, 1)]
        slabs = [pkg.api.KeySlab(kw.w.data_ptr() + c * kst[0], kw.kx.data_ptr() + c * kst[1], kw.ky.data_ptr() + c * kst[2],
                                 kz.data_ptr() + c * 208) for c in range(nc)]
        stream = ctx._stream()
        args = [(ctx._h, pt.data_ptr() + 16 * c * cap, keys.data_ptr() + 16 * c, 0, cap, lay, w.x.data_ptr() + c * cap * st[0],
                 w.y.data_ptr() + c * cap * st[1], w.z.data_ptr() + c * cap * st[2], w.ct.data_ptr() + 16 * c * cap, C.byref(slabs[c]),
                 reps[c].data_ptr(), stream) for c in range(nc)]

        def loop():
            for a_ in args:
                rc = ctx._lib.aesw_check_witness_device(*a_)
                assert rc == 0, rc

        t_one, t_loop = _alternate(torch, one, loop)
        print("\nK=14 N=1 C=4096 (%d blocks): one launch %.3f ms, %d one-circuit calls %.3f ms, ratio %.1f" % (n, t_one, nc, t_loop, t_loop / t_one))
        v = rep.cpu().tolist()
        assert v[:6] == [n, nc, 0, 0, 0, 0] and v[7] == 0
        assert not reps[:, 2:6].any().item()
        assert t_one < t_loop, (t_one, t_loop)
    finally:
        ctx.close()


def test_not_slower_than_the_per_block_key_check(gpu, pkg):
    """About 2^20 blocks (K = 20, N = 5, C = 256 full circuits): against the per-block-key check over the same number of blocks
    (its key slabs: one per block).  The many-circuit form reads 936 fewer HBM bytes per block and adds the scalar search:
    1.10 x is the 1 - 3 % drift between replays that DESIGN 5 records, plus the search."""
    torch = gpu
    ctx = pkg.Context(0)
    try:
        k, n_sets, nc = 20, 5, 256
        cap, keys, pt, kw, w, offs = _batch(torch, pkg, ctx, k, n_sets, nc, 2)
        n, lay = cap * nc, pkg.LAYOUT_PACKED
        rep = torch.empty(8, dtype=torch.int64, device="cuda")
        one = _one_launch(pkg, ctx, k, n_sets, nc, n, keys, pt, kw, w, offs, rep)
        pbk_keys = torch.repeat_interleave(keys, cap, dim=0)
        pw = ctx.encrypt_witness(pt, pbk_keys, layout=lay, want_ct=True, key_slab=True)
        rep7 = torch.empty(7, dtype=torch.int64, device="cuda")
        ks = pkg.api.KeySlab(*[t.data_ptr() for t in pw.key[:4]])
        pargs = (ctx._h, pt.data_ptr(), pbk_keys.data_ptr(), 1, n, lay, pw.x.data_ptr(), pw.y.data_ptr(), pw.z.data_ptr(), pw.ct.data_ptr(),
                 C.byref(ks), rep7.data_ptr(), ctx._stream())

        def pbk():
            rc = ctx._lib.aesw_check_witness_device(*pargs)
            assert rc == 0, rc

        t_one, t_pbk = _alternate(torch, one, pbk)
        print("\nK=20 N=5 C=256 (%d blocks): many-circuit check %.3f ms, per-block-key check %.3f ms, ratio %.3f" % (n, t_one, t_pbk, t_one / t_pbk))
        assert rep.cpu().tolist()[:6] == [n, nc, 0, 0, 0, 0] and rep7.cpu().tolist()[:6] == [n, n, 0, 0, 0, 0]
        assert t_one <= 1.10 * t_pbk, (t_one, t_pbk)
    finally:
        ctx.close()
