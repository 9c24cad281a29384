"""aesw_vals_check_device (libaesw_vals.so) on the GPU: a VALUES witness certified in one check launch.

The expectation is never the checker's own table: a satisfied witness is the product's own VALUES output, held next to what
Context.check_witness reports for the PACKED output of the same inputs; a corrupted one is rebuilt into a PACKED witness by
tests/vals_recon.py (copying along block_copy_graph, in numpy), uploaded, and certified by the existing
Context.check_witness(PACKED) -- the two reports must agree field for field."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import guarded as G
import vals_check_cases as vcs
from vals_recon import reconstruct

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("blocks", "keys", "lookup_failures", "copy_failures", "gate_failures", "input_failures", "first", "satisfied")


def _tables(pkg, name):
    return {"reference": None, "fips": pkg.fips_tables(), "random": G.random_tables(17)}[name]


class Case:
    """n blocks in one key mode: the product's VALUES witness (y, z, ct, key slab) on the device."""

    def __init__(self, pkg, ctx, mode, n, seed):
        import torch
        self.pkg, self.ctx, self.mode, self.n = pkg, ctx, mode, n
        self.pbk = mode == "per_block"
        rng = np.random.default_rng(seed)
        pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        keys = rng.integers(0, 256, (n, 16) if self.pbk else 16, dtype=np.uint8)
        if n > 1:
            pt[1] = 0xFF
            if self.pbk:
                keys[1] = 0  # reaches S_BOX[0xff]
        self.pt, self.keys = torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda()
        V = pkg.LAYOUT_VALUES
        if mode == "scheduled":
            self.kw = ctx.schedule_key(self.keys, layout=V)
            self.wit = ctx.encrypt_witness(self.pt, None, layout=V, want_ct=True)
        else:
            self.wit = ctx.encrypt_witness(self.pt, self.keys, layout=V, want_ct=True, key_slab=True)
            self.kw = self.wit.key
        self.ct = self.wit.ct
        torch.cuda.synchronize()

    def check(self, keys=True, ct=True):
        return self.ctx.check_values(self.pt, self.keys if keys or self.pbk else None, self.wit, self.kw, ct=self.ct if ct else None)

    def packed_reference(self, keys=True, ct=True):
        """What check_witness reports for the product's PACKED witness of the same inputs."""
        P = self.pkg.LAYOUT_PACKED
        if self.mode == "scheduled":
            kw = self.ctx.schedule_key(self.keys, layout=P)
            w = self.ctx.encrypt_witness(self.pt, None, layout=P, want_ct=True)
        else:
            w = self.ctx.encrypt_witness(self.pt, self.keys, layout=P, want_ct=True, key_slab=True)
            kw = w.key
        return self.ctx.check_witness(self.pt, self.keys if keys or self.pbk else None, w, kw, layout=P, ct=w.ct if ct else None)

    def raw(self, rep, stream=None, ct=None, keys=None):
        lib = self.pkg.api.load_vals_library()
        ks = self.pkg.api.KeySlab(*[t.data_ptr() for t in self.kw[:4]])
        rc = lib.aesw_vals_check_device(self.ctx._h, self.pt.data_ptr(), (self.keys if keys is None else keys).data_ptr(), 1 if self.pbk else 0, self.n,
                                        self.wit.y.data_ptr(), self.wit.z.data_ptr(), (self.ct if ct is None else ct).data_ptr(), C.byref(ks),
                                        rep.data_ptr(), self.ctx._stream() if stream is None else stream)
        assert rc == 0, rc


@pytest.mark.parametrize("tables", vcs.TABLE_SETS)
@pytest.mark.parametrize("mode", vcs.KEY_MODES)
def test_the_products_own_values_witness_is_satisfied(pkg, mode, tables):
    import torch
    ctx = pkg.Context(0, tables=_tables(pkg, tables))
    try:
        for n in vcs.SIZES:
            c = Case(pkg, ctx, mode, n, seed=n + len(mode))
            clean = {"blocks": n, "keys": n if c.pbk else 1, "lookup_failures": 0, "copy_failures": 0, "gate_failures": 0, "input_failures": 0,
                     "first": None, "satisfied": True}
            for keys in ((True, False) if mode == "scheduled" else (True,)):  # scheduled: d_keys given and NULL
                for ct in (True, False):
                    got = c.check(keys=keys, ct=ct)
                    assert got == clean, (mode, tables, n, keys, ct, got)
                    if n <= 4099:
                        assert got == c.packed_reference(keys=keys, ct=ct)
            rep = ctx.check_values(c.pt, c.keys, c.wit, c.kw, ct=c.ct, sync=False)
            torch.cuda.synchronize()
            assert tuple(rep.shape) == (7,) and pkg.api.check_report_dict(rep) == clean
        if tables != "reference":  # the tables are inputs of the check: the same bytes fail under the reference's
            other = pkg.Context(0)
            try:
                got = other.check_values(c.pt, c.keys, c.wit, c.kw, ct=c.ct)
                assert got["lookup_failures"] > 0 and got["input_failures"] == 0 and got["blocks"] == c.n
            finally:
                other.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", vcs.KEY_MODES)
def test_single_byte_corruptions_agree_with_the_packed_check_of_the_rebuilt_witness(pkg, ctx, mode):
    """300 seeded single-byte corruptions over y, z, the four key-slab columns, pt, ct and keys.  For each the values report
    equals, field for field, Context.check_witness(PACKED) on the witness numpy rebuilds from the same bytes."""
    import torch
    n = 41
    c = Case(pkg, ctx, mode, n, seed=500 + len(mode))
    P = pkg.LAYOUT_PACKED
    dev = {"y": c.wit.y, "z": c.wit.z, "kx": c.kw.kx, "ky": c.kw.ky, "kz": c.kw.kz, "w": c.kw.w, "pt": c.pt.view(-1), "ct": c.ct.view(-1),
           "keys": c.keys.view(-1)}
    host = {k_: v.cpu().numpy().copy() for k_, v in dev.items()}
    with_keys = mode != "scheduled"  # scheduled: half of the cases pass d_keys, half NULL

    def both(use_keys):
        got = c.check(keys=use_keys)
        x, y, z = reconstruct(pkg, host["pt"].reshape(n, 16), host["y"], host["z"], (host["w"], host["kx"], host["ky"], host["kz"]), c.pbk)
        w = pkg.Witness(*[torch.from_numpy(a).cuda() for a in (x, y, z)], None, None)
        want = ctx.check_witness(c.pt, c.keys if use_keys or c.pbk else None, w, c.kw, layout=P, ct=c.ct)
        return got, want

    got, want = both(True)
    assert got == want and got["satisfied"] and got["blocks"] == n
    rng = np.random.default_rng(900 + len(mode))
    names = list(dev)
    cases = [(name, int(rng.integers(0, host[name].size)), int(rng.integers(1, 256))) for name in names for _ in range(34)]
    assert len(cases) >= 300
    failing, seen = 0, set()
    for j, (name, i, v) in enumerate(cases):
        use_keys = with_keys or j % 2 == 0
        dev[name][i] ^= v
        host[name][i] ^= v
        try:
            got, want = both(use_keys)
        finally:
            dev[name][i] ^= v
            host[name][i] ^= v
        assert {f: got[f] for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, i, v, got, want)
        if name in ("y", "z", "pt", "ct"):
            assert got["copy_failures"] == 0 and got["gate_failures"] == 0 and not got["satisfied"], (name, i, got)
        if name == "ct":
            assert got["input_failures"] == 1 and got["first"][2] == 4 and 1344 <= got["first"][3] < 1360, got
        failing += not got["satisfied"]
        seen.add(name)
    assert seen == set(names) and failing >= 34 * 7, failing  # everything but an ignored key literal fails
    got, want = both(True)
    assert got == want and got["satisfied"]


def test_graph_replays_and_three_streams(pkg, ctx):
    """Captured into a hipGraph behind the launch that produces the witness and replayed three times into the same
    (re-poisoned) report: the eager report each time.  Then the same context on three streams at once: three equal reports."""
    import torch
    n = 4099
    c = Case(pkg, ctx, "per_block", n, seed=77)
    bad_ct, bad_keys = c.ct.clone(), c.keys.clone()
    bad_ct[3000, 5] ^= 0x20
    bad_keys[17, 2] ^= 1
    torch.cuda.synchronize()
    arena = G.DeviceArena(G.CANARIES[0])
    rep = arena.out("eager_report", 56)
    c.raw(rep, ct=bad_ct, keys=bad_keys)
    torch.cuda.synchronize()
    eager = pkg.api.check_report_dict(rep.view(torch.int64))
    assert eager["input_failures"] == 2 and eager["first"] == (17, True, 4, 2) and eager["blocks"] == n and eager["keys"] == n

    grep = arena.out("graph_report", 56)
    out = ctx.alloc_witness(n, pkg.LAYOUT_VALUES, want_ct=True, key_slab=True)
    made = Case.__new__(Case)
    made.pkg, made.ctx, made.n, made.pbk, made.pt, made.keys, made.wit, made.kw, made.ct = pkg, ctx, n, True, c.pt, c.keys, out, out.key, out.ct
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        ctx.encrypt_witness(c.pt, c.keys, layout=pkg.LAYOUT_VALUES, out=out)
        made.raw(grep, ct=bad_ct, keys=bad_keys)
    torch.cuda.synchronize()
    assert arena.poisoned(grep), "the captured call ran during capture"
    for _ in range(3):
        for t in (out.y, out.z, out.ct):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert pkg.api.check_report_dict(grep.view(torch.int64)) == eager
        grep.fill_(arena.canary)
    arena.check()

    streams = [torch.cuda.Stream() for _ in range(3)]
    reps = [arena.out("stream_report_%d" % i, 56) for i in range(3)]
    torch.cuda.synchronize()
    for s, r in zip(streams, reps):
        with torch.cuda.stream(s):
            c.raw(r, ct=bad_ct, keys=bad_keys)
    torch.cuda.synchronize()
    arena.check()
    for r in reps:
        assert pkg.api.check_report_dict(r.view(torch.int64)) == eager


def test_the_headline_size_with_per_block_keys(pkg, ctx):
    c = Case(pkg, ctx, "per_block", vcs.HEADLINE, seed=1)
    got = c.check()
    assert got["satisfied"] and got["first"] is None and got["blocks"] == got["keys"] == vcs.HEADLINE, got
    c.wit.z[(vcs.HEADLINE - 1) * 608 + 607] ^= 0x80  # the last cell of the last block
    got = c.check()
    assert got["first"] == (vcs.HEADLINE - 1, False, 1, 1359) and got["input_failures"] == 1 and got["lookup_failures"] == 1, got


@pytest.mark.parametrize("mode", ("shared", "per_block"))
def test_nothing_is_written_but_the_report(pkg, ctx, mode):
    import torch
    n = 67
    c = Case(pkg, ctx, mode, n, seed=5)
    for canary in G.CANARIES:
        arena = G.DeviceArena(canary)
        src = {"pt": c.pt, "keys": c.keys, "y": c.wit.y, "z": c.wit.z, "ct": c.ct, "w": c.kw.w, "kx": c.kw.kx, "ky": c.kw.ky, "kz": c.kw.kz}
        buf = {}
        for name, t in src.items():
            buf[name] = arena.out(name, t.numel())
            buf[name].copy_(t.reshape(-1))
        before = {name: t.cpu().numpy().copy() for name, t in buf.items()}
        rep = arena.out("report", 56)
        ks = pkg.api.KeySlab(*[buf[k_].data_ptr() for k_ in ("w", "kx", "ky", "kz")])
        torch.cuda.synchronize()
        rc = pkg.api.load_vals_library().aesw_vals_check_device(ctx._h, buf["pt"].data_ptr(), buf["keys"].data_ptr(), 1 if c.pbk else 0, n, buf["y"].data_ptr(),
                                                               buf["z"].data_ptr(), buf["ct"].data_ptr(), C.byref(ks), rep.data_ptr(), ctx._stream())
        assert rc == 0
        arena.check()
        for name, t in buf.items():
            G.assert_bytes(name, t.cpu().numpy(), before[name])
        got = pkg.api.check_report_dict(rep.view(torch.int64))
        assert got["satisfied"] and got["blocks"] == n and got["keys"] == (n if c.pbk else 1) and got["first"] is None


def test_argument_rules(pkg, ctx):
    import torch
    c = Case(pkg, ctx, "per_block", 5, seed=3)
    lib = pkg.api.load_vals_library()
    arena = G.DeviceArena(G.CANARIES[1])
    rep = arena.out("report", 56)
    ks = pkg.api.KeySlab(*[t.data_ptr() for t in c.kw[:4]])
    torch.cuda.synchronize()

    def call(ctx_h=None, pt=None, keys=c.keys.data_ptr(), n=c.n, y=c.wit.y.data_ptr(), z=c.wit.z.data_ptr(), ct=c.ct.data_ptr(), slab=ks, report=None):
        return lib.aesw_vals_check_device(ctx._h if ctx_h is None else ctx_h, c.pt.data_ptr() if pt is None else pt, keys, 1, n, y, z, ct,
                                          C.byref(slab) if slab is not None else None, rep.data_ptr() if report is None else report, ctx._stream())

    no_kz = pkg.api.KeySlab(c.kw.w.data_ptr(), c.kw.kx.data_ptr(), c.kw.ky.data_ptr(), None)
    bad_kz = pkg.api.KeySlab(c.kw.w.data_ptr(), c.kw.kx.data_ptr(), c.kw.ky.data_ptr(), c.kw.kz.data_ptr() + 8)
    for kw in (dict(y=None), dict(z=None), dict(slab=None), dict(slab=no_kz), dict(slab=bad_kz), dict(y=c.wit.y.data_ptr() + 4),
               dict(z=c.wit.z.data_ptr() + 8), dict(pt=c.pt.data_ptr() + 4), dict(ct=c.ct.data_ptr() + 4), dict(keys=None),
               dict(keys=c.keys.data_ptr() + 1), dict(report=rep.data_ptr() + 4)):
        assert call(**kw) == 1, kw  # AESW_ERR_INVALID_ARG
    g = pkg.Group([0])
    try:
        assert call(ctx_h=g._h) == 1
        with pytest.raises(pkg.AeswError):
            g.check_values(c.pt, c.keys, c.wit, c.kw)
    finally:
        g.close()
    torch.cuda.synchronize()
    assert arena.poisoned(rep), "a refused call launched something"
    assert call() == 0 and call(n=0, pt=0, y=None, z=None, ct=None) == 0  # n == 0: the report is reset, nothing is checked
    torch.cuda.synchronize()
    got = pkg.api.check_report_dict(rep.view(torch.int64))
    assert got["blocks"] == 0 and got["keys"] == 0 and got["satisfied"] and got["first"] is None
    assert lib.aesw_vals_prepare(ctx._h) == 0
    with pytest.raises(pkg.AeswError):  # the existing refusals of VALUES stay
        ctx.check_witness(c.pt, c.keys, c.wit, c.kw, layout=pkg.LAYOUT_VALUES)


def test_the_plain_c_example(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_vals_check"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_vals_check.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_vals", "-laesw", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    good = subprocess.run([str(exe), "4099"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert good.returncode == 0 and good.stdout.rstrip().endswith("ok"), good.stdout
    assert "4099 blocks + 4099 key slabs: 0 lookup, 0 copy, 0 gate, 0 literal failures" in good.stdout, good.stdout
    poked = subprocess.run([str(exe), "4099", "poke"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert poked.returncode not in (0, 2, 3) and poked.returncode > 0, poked.stdout
    assert "first: block 4098, lookup, row 40" in poked.stdout, poked.stdout
