"""The option table on a real context and on a group, and the warm-up aesw_create does for every launch a context can make.

Options: every name of tests/option_table.py EXPECTED (the options as they were before csrc/aesw_options.h described them once)
reads its default on a fresh context, takes its lowest and highest value and reads them back, and refuses the values next to its
range; the follow-ups a table row cannot express keep working (arena_cache 0, key_slots, the one-way force_table_path); a set on a
group reaches every member.  A group here has two members on device 0 (tests/test_gpu_group.py's GROUPS), so one GPU is enough.

Warm-up: one launch per encrypt_kernel and key_kernel instantiation of tests/kernel_cases.py, all captured into ONE graph on one
stream of a fresh context and replayed once: every instantiation launches from a capture with more than 48 KiB of dynamic LDS and
writes the oracle's bytes.  (What the test cannot see is WHO raised an instantiation's LDS limit, aesw_create or the launch itself:
the runtime does not refuse the attribute call under capture.)  The shapes are the smallest with a full group plus a tail wave and
dynamic LDS above 48 KiB: the layout's largest wave count w and 16 w + 1 blocks, and for key_kernel 4 waves with round keys and 65
keys."""
import ctypes as C

import numpy as np
import pytest

import guarded as G
import kernel_cases as kc
import option_table as ot

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = 1


def _refused(c, name, value):
    with pytest.raises(Exception) as e:
        c.set_option(name, value)
    assert getattr(e.value, "status", None) == ERR_INVALID_ARG, (name, value, e.value)


def _member_option(g, i, name):
    v = C.c_int64()
    assert g._lib.aesw_get_option(C.c_void_p(g.member_handle(i)), name.encode(), C.byref(v)) == 0, (i, name)
    return int(v.value)


def _options_hold(c, members=None):
    """Every row of EXPECTED on context (or group) `c`; members: (group, count) to look at every member behind a set."""
    def reads(name, want):
        assert c.get_option(name) == want, name
        if members:
            g, count = members
            assert [_member_option(g, i, name) for i in range(count)] == [want] * count, name

    for name, row in ot.EXPECTED.items():
        if not row.readable:  # "trace_ptr": not in this build, an unknown name
            _refused(c, name, 0)
            with pytest.raises(Exception):
                c.get_option(name)
            continue
        if row.default is not None:
            reads(name, row.default)
        else:
            assert 1 <= c.get_option(name) <= 4, name  # effective_copy_threads: a share of the CPUs, 1 ... 4
        if not row.settable:
            _refused(c, name, 0)
            _refused(c, name, 1)
    for name, row in ot.EXPECTED.items():
        if not row.settable or name == "force_table_path":
            continue
        for v in ot.inside(row):
            c.set_option(name, v)
            reads(name, (1 if v else 0) if row.form == "truthy" else v)
        keep = c.get_option(name)
        for v in ot.outside(row):
            _refused(c, name, v)
            reads(name, keep)
    # names that share a field
    c.set_option("store_mode", 2)
    reads("nt_stores", 0)
    c.set_option("nt_stores", 5)
    reads("store_mode", 1)
    # the follow-ups
    c.set_option("arena_cache", 0)
    reads("arena_cached_bytes", 0)
    c.set_option("key_slots", 7)
    reads("key_slots", 7)
    ftp = ot.EXPECTED["force_table_path"]  # takes any value; one way: 0 changes nothing, anything else is the table path for good
    reads("force_table_path", 0)
    c.set_option("force_table_path", 0)
    reads("force_table_path", 0)
    for v in (1, 0, ftp.lo, ftp.hi, 0):
        c.set_option("force_table_path", v)
        reads("force_table_path", 1)
    assert not c.uses_xtime_path
    _refused(c, "no_such_option", 0)
    with pytest.raises(Exception):
        c.get_option("no_such_option")


def test_options_on_a_context_and_on_a_group(pkg):
    c = pkg.Context(0)
    try:
        _options_hold(c)
    finally:
        c.close()
    g = pkg.Group([0, 0])
    try:
        assert g.size == 2
        _options_hold(g, members=(g, 2))
    finally:
        g.close()


def test_warm_up_covers_every_launch(pkg, oracle):
    import torch
    c = pkg.Context(0)  # fresh: nothing launched on it, every attribute it has was set by aesw_create
    try:
        assert c.uses_xtime_path
        rng = np.random.default_rng(0x0A17)
        n_max = kc.BPW * 4 + 1
        pt = rng.integers(0, 256, (n_max, 16), dtype=np.uint8)
        keys = rng.integers(0, 256, (n_max, 16), dtype=np.uint8)
        pt[1], keys[1] = 0xFF, 0  # S_BOX[255]
        dpt, dkeys = torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda()
        dkey0 = dkeys[0].contiguous()
        # the scheduled key of the "scheduled" cases: eager, on the stream the capture will use (a captured scheduled-key launch is
        # ordered behind its key by stream order; on another stream only the first one could be), finished before the capture
        cap = torch.cuda.Stream()
        with torch.cuda.stream(cap):
            c.schedule_key(dkey0, key_slab=False)
        torch.cuda.synchronize()
        # outputs of every launch, allocated (and poisoned) before the capture
        enc, key = [], []
        for layout, xt, form, nt in kc.ENCRYPT_CASES:
            n = kc.BPW * kc.max_waves(layout) + 1
            pbk = form.startswith("pbk")
            out = c.alloc_witness(n, layout, want_ct=True, key_slab=form in ("shared", "pbk_slab"), n_keys=n if pbk else 1)
            enc.append((layout, xt, form, nt, n, out))
        for layout, xt, nt in kc.KEY_CASES:
            a = G.DeviceArena()
            key.append((layout, xt, nt, a.key_witness(pkg, n_max, layout, want_rk=True)))
        for *_case, out in enc:
            for t in list(out[:4]) + (list(out.key[:4]) if out.key is not None else []):
                t.fill_(0xEE)
        torch.cuda.synchronize()

        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            for xt in (True, False):  # the reference tables through the generic path compute the same bytes
                if not xt:
                    c.set_option("force_table_path", 1)
                for layout, cxt, form, nt, n, out in enc:
                    if cxt != xt:
                        continue
                    pbk = form.startswith("pbk")
                    c.set_option("store_mode", nt)
                    c.set_option("waves_pbk" if pbk else "waves_shared", kc.max_waves(layout))
                    c.encrypt_witness(dpt[:n], None if form == "scheduled" else (dkeys[:n] if pbk else dkey0), layout=layout, out=out)
                c.set_option("waves_pbk", 4)
                for layout, cxt, nt, out in key:
                    if cxt != xt:
                        continue
                    c.set_option("key_store_mode", nt)
                    G.key_schedule(c, dkeys, layout, out)
        graph.replay()
        torch.cuda.synchronize()

        exp = {}
        for layout in kc.LAYOUTS:
            n = kc.BPW * kc.max_waves(layout) + 1
            exp[layout, False] = oracle.encrypt_witness(pt[:n], keys[0], layout=layout)
            exp[layout, True] = oracle.encrypt_witness(pt[:n], keys[:n], layout=layout)
            exp[layout, "slab1"] = oracle.key_schedule_witness(keys[0], layout=layout)
            exp[layout, "slabs"] = oracle.key_schedule_witness(keys, layout=layout)
        for layout, xt, form, nt, n, out in enc:
            what = "encrypt %s %s %s nt=%d" % (kc.LAYOUT_NAME[layout], "xt" if xt else "generic", form, nt)
            e = exp[layout, form.startswith("pbk")]
            for col in ("x", "y", "z", "ct"):
                G.assert_bytes("%s %s" % (what, col), getattr(out, col).cpu().numpy(), getattr(e, col))
            if out.key is not None:
                ke = exp[layout, "slabs" if form == "pbk_slab" else "slab1"]
                for col in ("w", "kx", "ky", "kz"):
                    want = getattr(ke, col)
                    G.assert_bytes("%s %s" % (what, col), getattr(out.key, col).cpu().numpy(), want.reshape(-1)[:getattr(out.key, col).numel()])
        for layout, xt, nt, out in key:
            what = "key_kernel %s %s nt=%d" % (kc.LAYOUT_NAME[layout], "xt" if xt else "generic", nt)
            for col in ("w", "kx", "ky", "kz", "rk"):
                G.assert_bytes("%s %s" % (what, col), getattr(out, col).cpu().numpy(), getattr(exp[layout, "slabs"], col))
    finally:
        c.close()
