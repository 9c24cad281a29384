"""Every kernel instantiation of libaesw.so, launched into poisoned, guard-banded outputs and compared byte for byte with the
CPU oracle (tests/guarded.py; the case table and the dispatch rules it stands on are tests/kernel_cases.py, and
tests/test_instantiation_coverage.py holds the table against the library's symbols).

Each case has its own Context, closed in `finally`.  Expected values come from an oracle built with the context's tables.  An
output the kernel did not write keeps its canary, a write past an output damages its guard band; ragged sizes around every
group size, both canaries at least once per case."""
import numpy as np
import pytest

import guarded as G
import kernel_cases as kc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

SEED = 0x1A57


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if n > 1:
        pt[1], keys[1] = 0xFF, 0  # pt ^ key == 0xff: S_BOX[255], where the reference's table differs from FIPS
    return pt, keys


def _context(pkg, xt):
    tables = None if xt else G.random_tables()
    c = pkg.Context(0, tables=tables)
    assert c.uses_xtime_path == xt
    return c, ol.Oracle(tables=tables)


def _ids(case):
    return "-".join(kc.LAYOUT_NAME[v] if i == 0 else (("xt" if v else "generic") if isinstance(v, bool) else str(v))
                    for i, v in enumerate(case))


def _cmp(name, got, exp):
    G.assert_bytes(name, got.cpu().numpy() if hasattr(got, "cpu") else got, exp)


def run_encrypt(c, pkg, orc, layout, form, n, canary, seed, check=True):
    """One encrypt launch of key form `form` into a guarded Witness (ct and key slab always requested: shared keys through the
    fused launch, a scheduled key through aesw_schedule_key_device); guards, bytes, and check_witness on dense / packed."""
    import torch
    pt, keys = _inputs(n, seed)
    a = G.DeviceArena(canary)
    dpt = a.input("pt", pt)
    pbk = form.startswith("pbk")
    k_host = keys if pbk else keys[0]
    dkey = a.input("keys", k_host)
    if form == "scheduled":
        slab = a.key_witness(pkg, 1, layout, want_rk=False)
        G.schedule_key(c, pkg, dkey, layout, slab)
        out = a.witness(pkg, n, layout, want_ct=True, key_slab=False)
        c.encrypt_witness(dpt, None, layout=layout, out=out)
    else:
        out = a.witness(pkg, n, layout, want_ct=True, key_slab=form != "pbk", n_keys=n if pbk else 1)
        c.encrypt_witness(dpt, dkey, layout=layout, out=out)
        slab = out.key
    a.check()
    what = "%s %s n=%d canary 0x%02x" % (kc.LAYOUT_NAME[layout], form, n, canary)
    exp = orc.encrypt_witness(pt, k_host, layout=layout, threads=4)
    for col in "xyz":
        _cmp("%s %s" % (what, col), getattr(out, col), getattr(exp, col))
    _cmp(what + " ct", out.ct, exp.ct)
    kexp = orc.key_schedule_witness(k_host, layout=layout, threads=4)
    if slab is not None:
        for col in ("w", "kx", "ky", "kz"):
            _cmp("%s %s" % (what, col), getattr(slab, col), getattr(kexp, col))
    if check and layout != kc.VALUES:
        if slab is None:  # per-block keys without a slab: the oracle's slabs, uploaded
            slab = pkg.KeyWitness(*[torch.from_numpy(getattr(kexp, col)).cuda() for col in ("w", "kx", "ky", "kz")], None)
        rep = c.check_witness(dpt, dkey, out, slab, layout=layout, ct=out.ct)
        assert rep["satisfied"] and rep["blocks"] == n, (what, rep)
    return a, out


# ---- encrypt_kernel: one case per instantiation -------------------------------------------------------------------------

@pytest.mark.parametrize("layout,xt,form,nt", kc.ENCRYPT_CASES, ids=[_ids(v) for v in kc.ENCRYPT_CASES])
def test_encrypt_instantiation(pkg, layout, xt, form, nt):
    c, orc = _context(pkg, xt)
    try:
        c.set_option("store_mode", nt)
        pbk = form.startswith("pbk")
        for waves in range(1, kc.max_waves(layout) + 1):
            c.set_option("waves_pbk" if pbk else "waves_shared", waves)
            assert c.get_option("effective_waves_pbk" if pbk else "effective_waves_shared") == kc.auto_waves(
                kc.PACKED, pbk, waves, waves)
            for i, n in enumerate(kc.encrypt_sizes(waves)):
                # 17 is ragged for every wave count: both canaries; other sizes alternate
                for canary in (G.CANARIES if n == 17 else (G.CANARIES[(i + waves) % 2],)):
                    run_encrypt(c, pkg, orc, layout, form, n, canary, SEED + 131 * n + waves)
    finally:
        c.close()


# ---- key_kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,xt,nt", kc.KEY_CASES, ids=[_ids(v) for v in kc.KEY_CASES])
def test_key_kernel_instantiation(pkg, layout, xt, nt):
    c, orc = _context(pkg, xt)
    try:
        c.set_option("key_store_mode", nt)
        i = 0
        for want_rk in (True, False):
            for wp in kc.KEY_WAVES_PBK:
                c.set_option("waves_pbk", wp)
                assert c.get_option("effective_waves_key") == kc.auto_waves_key(kc.PACKED, False, wp)
                waves = kc.auto_waves_key(layout, want_rk, wp)
                for n in kc.key_sizes(waves):
                    remap = kc.KEY_REMAPS[i % len(kc.KEY_REMAPS)]
                    c.set_option("xcd_remap", remap)
                    canary = G.CANARIES[i % 2]
                    i += 1
                    _, keys = _inputs(n, SEED + 7 * n + wp)
                    a = G.DeviceArena(canary)
                    dk = a.input("keys", keys)
                    out = a.key_witness(pkg, n, layout, want_rk=want_rk)
                    G.key_schedule(c, dk, layout, out)
                    a.check()
                    exp = orc.key_schedule_witness(keys, layout=layout, threads=4)
                    what = "%s rk=%s waves=%d n=%d remap=%d canary 0x%02x" % (kc.LAYOUT_NAME[layout], want_rk, waves, n, remap, canary)
                    for col in ("w", "kx", "ky", "kz") + (("rk",) if want_rk else ()):
                        _cmp("%s %s" % (what, col), getattr(out, col), getattr(exp, col))
    finally:
        c.close()


# ---- striding workgroups and the XCD remap -----------------------------------------------------------------------------

@pytest.mark.parametrize("cap,remap", kc.STRIDE_CASES, ids=["cap%d-remap%d" % v for v in kc.STRIDE_CASES])
def test_striding_and_remap(pkg, cap, remap):
    """grid_cap x xcd_remap for every key form: group counts below one turn of 8*C groups, on one turn and past it with a
    tail (launch_encrypt drops the remap when grid_cap % 8 != 0: those are exact too)."""
    orc = ol.Oracle()
    for layout, waves in kc.STRIDE_LAYOUTS:
        c = pkg.Context(0)
        try:
            c.set_option("grid_cap", cap)
            c.set_option("xcd_remap", remap)
            if waves:
                c.set_option("waves_shared", waves)
                c.set_option("waves_pbk", waves)
            for form in kc.KEY_FORMS:
                bpg = kc.BPW * kc.auto_waves(layout, form.startswith("pbk"), waves, waves)
                for j, groups in enumerate(kc.stride_group_counts(cap, remap)):
                    n = (groups - 1) * bpg + 1 + (groups * 7) % bpg  # a ragged last group
                    run_encrypt(c, pkg, orc, layout, form, n, G.CANARIES[j % 2], SEED + groups, check=False)
        finally:
            c.close()


def test_lds_pad(pkg):
    orc = ol.Oracle()
    c = pkg.Context(0)
    try:
        c.set_option("lds_pad", kc.LDS_PAD)
        for layout in kc.LAYOUTS:
            for form in kc.KEY_FORMS:
                for n in (17, 3 * 48 + 5):
                    run_encrypt(c, pkg, orc, layout, form, n, G.CANARIES[n % 2], SEED + n)
    finally:
        c.close()


# ---- assemble, expand_fr, the lookup table ----------------------------------------------------------------------------------

def _fr_lut():
    from test_gpu_round4 import _fr_lut as lut
    return lut()


@pytest.mark.parametrize("k,n_sets,spare", kc.ASSEMBLE_SHAPES, ids=["k%d-n%d-spare%d" % v for v in kc.ASSEMBLE_SHAPES])
def test_assemble_instantiations(pkg, oracle, k, n_sets, spare):
    """Every assemble_geometry x fr_store_mode x {bytes, Fr} into a guarded, poisoned `out`, against the restated synthesize()
    (K >= 11) or the clipped key slab (K < 11) -- the expectation of test_gpu_round4's boundary test."""
    from test_gpu_round4 import _small_k_expectation
    lut = _fr_lut()
    n = pkg.block_capacity(k, n_sets) - spare
    rng = np.random.default_rng(1000 + k)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    pts = rng.integers(0, 256, (max(n, 1), 16), dtype=np.uint8)
    c = pkg.Context(0)
    try:
        src = G.DeviceArena()
        kw = src.key_witness(pkg, 1, pkg.LAYOUT_PACKED, want_rk=False)
        G.schedule_key(c, pkg, src.input("key", key), pkg.LAYOUT_PACKED, kw)
        wit = src.witness(pkg, max(n, 1), pkg.LAYOUT_PACKED, want_ct=False, key_slab=False)
        c.encrypt_witness(src.input("pt", pts), None, layout=pkg.LAYOUT_PACKED, out=wit)
        src.check()
        if k >= 11:
            with oracle.circuit(k, n_sets, key, pts[:n], record_copies=False) as circ:
                assert circ.status == 0
                expect = np.stack([circ.advice(col) for col in range(3 * n_sets + 1)])
        else:
            expect = _small_k_expectation(oracle, k, n_sets, key)
        ncol = 3 * n_sets + 1
        i = 0
        for geo in kc.ASSEMBLE_GEOMETRIES:
            c.set_option("assemble_geometry", geo)
            for nt in kc.STORE_MODES:
                c.set_option("fr_store_mode", nt)
                for as_fr in (False, True):
                    a = G.DeviceArena(G.CANARIES[i % 2])
                    i += 1
                    shape = (ncol, 1 << k, 32) if as_fr else (ncol, 1 << k)
                    out = a.out("advice", int(np.prod(shape)), shape)
                    assert a.poisoned(out)
                    c.assemble_advice(k, n_sets, wit, kw, n, layout=pkg.LAYOUT_PACKED, as_fr=as_fr, out=out)
                    a.check()
                    what = "geo %d mode %d as_fr %s (%s)" % (geo, nt, as_fr, kc.assemble_kernel(geo, nt, as_fr, k, n_sets))
                    _cmp(what, out, lut[expect] if as_fr else expect)
    finally:
        c.close()


@pytest.mark.parametrize("geo,nt", kc.EXPAND_CASES, ids=["geo%d-mode%d" % v for v in kc.EXPAND_CASES])
def test_expand_fr_instantiation(pkg, geo, nt):
    lut = _fr_lut()
    c = pkg.Context(0)
    try:
        c.set_option("fr_geometry", geo)
        c.set_option("fr_store_mode", nt)
        for j, n_cells in enumerate(kc.EXPAND_SIZES):
            cells = np.random.default_rng(n_cells).integers(0, 256, n_cells, dtype=np.uint8)
            cells[: min(n_cells, 256)] = np.arange(min(n_cells, 256), dtype=np.uint8)
            a = G.DeviceArena(G.CANARIES[j % 2])
            out = a.out("fr", n_cells * 32, (n_cells, 32))
            c.expand_fr(a.input("cells", cells), out)
            a.check()
            _cmp("expand_fr geo %d mode %d n %d" % (geo, nt, n_cells), out, lut[cells])
    finally:
        c.close()


@pytest.mark.parametrize("xt", [True, False], ids=["xt", "generic"])
def test_lookup_table_guarded(pkg, xt):
    c, orc = _context(pkg, xt)
    try:
        for canary in G.CANARIES:
            a = G.DeviceArena(canary)
            cols = [a.out("t%d" % i, ol.TABLE_ROWS) for i in range(4)]
            G.lookup_table(c, cols)
            a.check()
            exp = orc.lookup_table()
            for i in range(4):
                _cmp("table column %d canary 0x%02x" % (i, canary), cols[i], exp[i])
    finally:
        c.close()


# ---- the host entry point ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,threads,pinned", kc.HOST_CASES, ids=[_ids(v) for v in kc.HOST_CASES])
def test_host_entry_point_guarded(pkg, layout, threads, pinned):
    """aesw_encrypt_witness into guarded pageable / page-locked outputs: chunked (chunk_blocks 1000, n = 2 x 1000 + 77),
    per-block keys with key slab and ct, copy_threads 1 / 4."""
    orc = ol.Oracle()
    c = pkg.Context(0)
    a = G.HostArena(G.CANARIES[threads % 2], pinned=pinned, pkg=pkg)
    try:
        c.set_option("chunk_blocks", kc.HOST_CHUNK)
        c.set_option("copy_threads", threads)
        n = kc.HOST_N
        pt, keys = _inputs(n, SEED + threads)
        wit = G.host_witness(a, pkg, n, layout, n_keys=n)
        G.encrypt_witness_host(c, pkg, pt, keys, n, layout, wit)
        a.check()
        exp = orc.encrypt_witness(pt, keys, layout=layout)
        kexp = orc.key_schedule_witness(keys, layout=layout)
        for col in "xyz":
            _cmp(col, getattr(wit, col), getattr(exp, col))
        _cmp("ct", wit.ct, exp.ct)
        for col in ("w", "kx", "ky", "kz"):
            _cmp(col, getattr(wit.key, col), getattr(kexp, col))
    finally:
        a.close()
        c.close()


# ---- the harness itself ---------------------------------------------------------------------------------------------------

def test_harness_detects_an_under_launch_and_a_write_past_a_view(pkg):
    """Not vacuous: (1) encrypt n-5 blocks into outputs sized and poisoned for n -- the n-block comparison fails, and only in
    the last five blocks' bytes of every column; (2) a byte written from the host one past a guarded view is reported."""
    import torch
    orc = ol.Oracle()
    c = pkg.Context(0)
    try:
        n = 53
        for layout in kc.LAYOUTS:
            pt, keys = _inputs(n, SEED)
            a = G.DeviceArena()
            out = a.witness(pkg, n, layout, want_ct=True, key_slab=False)
            c.encrypt_witness(a.input("pt", pt[: n - 5]), a.input("keys", keys[: n - 5]), layout=layout, out=out)
            a.check()  # nothing outside the views
            exp = orc.encrypt_witness(pt, keys, layout=layout)
            for col, stride in zip("xyzc", [pkg.column_stride(layout, i) for i in range(3)] + [16]):
                got = (out.ct if col == "c" else getattr(out, col)).cpu().numpy().reshape(-1)
                e = (exp.ct if col == "c" else getattr(exp, col)).reshape(-1)
                if not stride:
                    continue
                with pytest.raises(AssertionError):
                    G.assert_bytes(col, got, e)
                bad = np.nonzero(got != e)[0]
                assert bad.min() >= (n - 5) * stride, (layout, col, int(bad.min()))
                assert (got[(n - 5) * stride:] == a.canary).all()  # the tail still holds the poison
                assert np.array_equal(got[: (n - 5) * stride], e[: (n - 5) * stride])
        # a host write one byte past the end of a view
        a = G.DeviceArena()
        a.out("victim", 1000)
        a.check()
        buf, lo, nbytes = a._bufs["victim"]
        buf[lo + nbytes: lo + nbytes + 1].copy_(torch.tensor([a.canary ^ 0xFF], dtype=torch.uint8))
        with pytest.raises(AssertionError, match=r"victim: guard damaged at offset 1000 of the 1000-byte view"):
            a.check()
        # and one before the start
        a = G.DeviceArena(G.CANARIES[1])
        a.out("front", 64)
        buf, lo, _ = a._bufs["front"]
        buf[lo - 1: lo].copy_(torch.tensor([0], dtype=torch.uint8))
        with pytest.raises(AssertionError, match=r"front: guard damaged at offset -1 "):
            a.check()
    finally:
        c.close()
