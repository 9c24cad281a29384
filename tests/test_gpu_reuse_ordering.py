"""Reuse of device memory across calls on different streams: the ring of round-key slots and the placement cache of arenas.

In two places the library hands bytes that one call used to a later call: a schedule takes a round-key slot again
(aesw_schedule_key*, "key_slots"), and aesw_columns_alloc hands out an arena that aesw_columns_free put into its cache.
include/aesw.h orders both behind the earlier call's device work.  Natural timing almost never shows a hole there, so these
tests make the timing deterministic: stream A is held by a calibrated, bounded spin (torch.cuda._sleep) in front of its call,
and the contested call is enqueued on stream B while A's call is still pending.  That B really runs beside A is asserted, not
assumed: an event recorded on B just before the contested call completes before the event recorded on A behind its call.
Every output is compared with the oracle under the key it must carry; a mismatch names the key whose bytes were found."""
import numpy as np
import pytest

import guarded
import oracle_lib as ol

pytestmark = pytest.mark.gpu

THREADS = 16
L = ol.PACKED               # == pkg.LAYOUT_PACKED
CAL_CYCLES = 1 << 20        # the calibration spin (shader clocks)
TARGET_MS = 100.0           # one delay: long against the host calls it has to cover (microseconds each)
MAX_MS = 500.0              # no delay longer than this at the calibrated clock ...
MAX_CYCLES = 1 << 28        # ... nor at any shader clock from 537 MHz up (112 ms at the 2.4 GHz peak)
PROBE_STREAMS = 8


class Delay:
    """A bounded spin of the shader clock on one stream.  torch.cuda._sleep counts clocks, not time: calibrated once per
    session against timing events.  The spin waits on nothing but the clock."""

    def __init__(self, torch):
        self.torch = torch
        torch.cuda._sleep(CAL_CYCLES)  # the first launch loads the kernel
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(CAL_CYCLES)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        per = sorted(ms)[1]
        assert per > 0, ms
        self.cycles = max(1, min(int(CAL_CYCLES * TARGET_MS / per), int(CAL_CYCLES * MAX_MS / per), MAX_CYCLES))
        self.ms = self.cycles * per / CAL_CYCLES

    def hold(self, stream):
        """Everything enqueued on `stream` from now on runs about self.ms later."""
        with self.torch.cuda.stream(stream):
            self.torch.cuda._sleep(self.cycles)

    def free_stream(self, a):
        """A fresh stream whose work runs while `a` is held.  Streams may share a hardware queue (the runtime opens a few per
        process, and the context owns five streams of its own): probe up to PROBE_STREAMS fresh streams behind one delay on
        `a` and take the first whose event completes while `a` is still held."""
        torch = self.torch
        cands = [torch.cuda.Stream() for _ in range(PROBE_STREAMS)]
        self.hold(a)
        a_done = torch.cuda.Event()
        a_done.record(a)
        probes = []
        for s in cands:
            e = torch.cuda.Event()
            e.record(s)
            probes.append(e)
        found = None
        while found is None and not a_done.query():  # bounded: a_done completes when the delay ends
            for s, e in zip(cands, probes):
                if e.query():
                    if not a_done.query():  # (asked after the probe: the probe completed while A was held)
                        found = s
                    break
        a_done.synchronize()
        if found is None:
            pytest.fail("none of %d fresh streams ran while another stream was held for %.0f ms: every one is serialised behind "
                        "it, so this machine cannot exercise the reuse races" % (PROBE_STREAMS, self.ms))
        return found

    def assert_overlap(self, ev_b_before, ev_a_end, what):
        dt = ev_b_before.elapsed_time(ev_a_end)
        assert dt > 0, ("%s: stream B reached the contested call %.3f ms after stream A's delayed call ended (delay %.0f ms): "
                        "B was serialised behind A and the race was not exercised" % (what, -dt, self.ms))


def _warm(pkg, torch):
    """Every entry point and kernel the cases use, once, on a context of its own: first launches (code loading) stay out of
    the delay windows, and the cases' own contexts stay fresh."""
    c = pkg.Context(0)
    try:
        rng = np.random.default_rng(1)
        n = 2 * 48
        pt = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        keys = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        c.set_option("batch_streams", 3)
        c.schedule_key(keys[0].contiguous(), key_slab=True)
        c.encrypt_witness(pt, None, want_ct=True)
        c.encrypt_witness(pt, keys, want_ct=True, key_slab=True)
        c.encrypt_witness_batches([(pt[i * 32:(i + 1) * 32], None, c.alloc_witness(32, want_ct=True)) for i in range(3)],
                                  per_block_keys=False)
        c.schedule_key_host(np.zeros(16, np.uint8))
        c.encrypt_witness_host(pt.cpu().numpy(), None, want_ct=True)
        torch.cuda.synchronize()
    finally:
        c.close()


@pytest.fixture(scope="module")
def delay(pkg):
    import torch
    _warm(pkg, torch)
    return Delay(torch)


class _Under:
    """The oracle's witness (and key slab) of `pt` under one key or per-block key set, computed on first use."""

    def __init__(self, oracle, pt, name, key):
        self.oracle, self.pt, self.name, self.key = oracle, pt, name, key
        self._w = self._k = None

    def witness(self):
        if self._w is None:
            self._w = self.oracle.encrypt_witness(self.pt, self.key, layout=L, threads=THREADS)
        return self._w

    def slab(self):
        if self._k is None:
            self._k = self.oracle.key_schedule_witness(self.key, layout=L, threads=THREADS)
        return self._k


ENC = ("x", "y", "z", "ct")
SLAB = ("w", "kx", "ky", "kz")


def _snap(w, cols):
    """Host copies of the named members of a witness or key slab.  The comparisons (and the arguments a failure report
    prints) hold these, never device views: an arena's views die with its context."""
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)  # noqa: E731
    return {c: host(getattr(w, c)).reshape(-1) for c in cols}


def _enc_cols(w, lo, hi):
    sx, sy, sz = ol.ENC_STRIDE[L]
    f = lambda a: np.asarray(a).reshape(-1)  # noqa: E731
    return {"x": f(w.x)[lo * sx:hi * sx], "y": f(w.y)[lo * sy:hi * sy], "z": f(w.z)[lo * sz:hi * sz], "ct": f(w.ct)[lo * 16:hi * 16]}


def _slab_cols(k):
    return {c: np.asarray(getattr(k, c)).reshape(-1) for c in SLAB}


def _check(what, got, want, suspects, cols_of):
    exp = cols_of(want)
    for col, e in exp.items():
        g = got[col]
        d = guarded.first_diff(g, e)
        if d:
            whose = [s.name for s in suspects if np.array_equal(g, cols_of(s)[col])]
            raise AssertionError("%s, column %s: not the bytes of %s (%s)%s" % (
                what, col, want.name, d, "; they are the bytes of %s" % whose[0] if whose else ""))


def _carries(what, got, want, suspects=(), lo=0, hi=None):
    """x, y, z and ct of `got` (_snap) are the oracle's for blocks [lo, hi) of the batch under `want`'s key."""
    hi = want.pt.shape[0] if hi is None else hi
    _check(what, got, want, suspects, lambda u: _enc_cols(u.witness(), lo, hi))


def _slab_is(what, got, want, suspects=()):
    _check(what, got, want, suspects, lambda u: _slab_cols(u.slab()))


def _keys(rng, count, n=None):
    return [rng.integers(0, 256, (16,) if n is None else (n, 16), dtype=np.uint8) for _ in range(count)]


def test_one_slot_schedule_is_ordered_behind_the_pending_writer(pkg, oracle, delay):
    """key_slots = 1.  schedule(k1) on stream A, held by the delay; schedule(k2) on stream B, which runs beside A, and a
    scheduled-key launch on B right behind it.  The one slot is taken again while A's key kernel is still queued: B's key
    kernel must run behind it, or A's lands on top and every later scheduled-key launch encrypts with k1.  Launches on B, on a
    third stream, through the batch entry point (three internal streams) and through the host-pointer path all carry k2,
    the key of the last schedule that returned; each schedule's key slab is its own key's.  Exactly one schedule waited for
    another stream's writer, none for a reader."""
    import torch
    rng = np.random.default_rng(4101)
    n = 5000
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    k1, k2 = _keys(rng, 2)
    u1, u2 = _Under(oracle, pt, "k1", k1), _Under(oracle, pt, "k2", k2)
    u2.witness()
    c = pkg.Context(0)
    try:
        c.set_option("key_slots", 1)
        c.set_option("batch_streams", 3)
        arena = guarded.DeviceArena(guarded.CANARIES[0])
        dpt, dk1, dk2 = (torch.from_numpy(a).cuda() for a in (pt, k1, k2))
        slab1, slab2 = (arena.key_witness(pkg, 1, pkg.LAYOUT_PACKED, want_rk=False) for _ in range(2))
        outs = {s: arena.witness(pkg, n, pkg.LAYOUT_PACKED, key_slab=False) for s in ("B, right behind the schedule", "B", "C")}
        cuts = [0, 1234, 3234, n]
        spans = list(zip(cuts, cuts[1:]))
        bouts = [arena.witness(pkg, hi - lo, pkg.LAYOUT_PACKED, key_slab=False) for lo, hi in spans]
        a = torch.cuda.Stream()
        b = delay.free_stream(a)
        cs = torch.cuda.Stream()
        torch.cuda.synchronize()
        w0, r0 = c.get_option("key_writer_waits"), c.get_option("key_reader_waits")
        ev_a_end, ev_b_before = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        delay.hold(a)
        with torch.cuda.stream(a):
            guarded.schedule_key(c, pkg, dk1, pkg.LAYOUT_PACKED, slab1)
        ev_a_end.record(a)
        ev_b_before.record(b)
        with torch.cuda.stream(b):
            guarded.schedule_key(c, pkg, dk2, pkg.LAYOUT_PACKED, slab2)
            c.encrypt_witness(dpt, None, out=outs["B, right behind the schedule"], want_ct=True)
        torch.cuda.synchronize()
        delay.assert_overlap(ev_b_before, ev_a_end, "schedule(k2) on B")
        with torch.cuda.stream(b):
            c.encrypt_witness(dpt, None, out=outs["B"], want_ct=True)
        with torch.cuda.stream(cs):
            c.encrypt_witness(dpt, None, out=outs["C"], want_ct=True)
            c.encrypt_witness_batches([(dpt[lo:hi], None, o) for (lo, hi), o in zip(spans, bouts)], per_block_keys=False)
        host = c.encrypt_witness_host(pt, None, want_ct=True)
        torch.cuda.synchronize()
        arena.check()
        _slab_is("key slab of schedule(k1)", _snap(slab1, SLAB), u1, [u2])
        _slab_is("key slab of schedule(k2)", _snap(slab2, SLAB), u2, [u1])
        for where, w in outs.items():
            _carries("scheduled-key launch on %s" % where, _snap(w, ENC), u2, [u1])
        for (lo, hi), w in zip(spans, bouts):
            _carries("batch of blocks [%d, %d)" % (lo, hi), _snap(w, ENC), u2, [u1], lo, hi)
        _carries("host-pointer encrypt", _snap(host, ENC), u2, [u1])
        assert c.get_option("key_writer_waits") - w0 == 1 and c.get_option("key_reader_waits") == r0
    finally:
        torch.cuda.synchronize()
        c.close()


def test_ring_of_four_wraps_onto_a_pending_writer(pkg, oracle, delay):
    """The default ring of four slots.  schedule(k1) on stream A, held by the delay; on stream B four schedules k2 ... k5,
    each followed by a launch.  k2 ... k4 take fresh slots; k5 wraps onto k1's slot while A's key kernel is still queued
    and must run behind it.  Every launch carries its own key, and after a synchronise launches on B and on a third stream
    carry k5.  Only the wrapping schedule waited for another stream's writer."""
    import torch
    rng = np.random.default_rng(4102)
    n = 3000
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = _keys(rng, 5)
    us = [_Under(oracle, pt, "k%d" % (i + 1), k) for i, k in enumerate(keys)]
    for u in us[1:]:
        u.witness()
    c = pkg.Context(0)
    try:
        assert c.get_option("key_slots") == 4
        arena = guarded.DeviceArena(guarded.CANARIES[1])
        dpt = torch.from_numpy(pt).cuda()
        dkeys = [torch.from_numpy(k).cuda() for k in keys]
        slabs = [arena.key_witness(pkg, 1, pkg.LAYOUT_PACKED, want_rk=False) for _ in keys]
        outs = [arena.witness(pkg, n, pkg.LAYOUT_PACKED, key_slab=False) for _ in keys[1:]]
        after = [arena.witness(pkg, n, pkg.LAYOUT_PACKED, key_slab=False) for _ in range(2)]
        a = torch.cuda.Stream()
        b = delay.free_stream(a)
        cs = torch.cuda.Stream()
        torch.cuda.synchronize()
        w0, r0 = c.get_option("key_writer_waits"), c.get_option("key_reader_waits")
        ev_a_end, ev_b_before = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        delay.hold(a)
        with torch.cuda.stream(a):
            guarded.schedule_key(c, pkg, dkeys[0], pkg.LAYOUT_PACKED, slabs[0])
        ev_a_end.record(a)
        waits = []
        for j in range(1, 5):
            if j == 4:
                ev_b_before.record(b)
            with torch.cuda.stream(b):
                guarded.schedule_key(c, pkg, dkeys[j], pkg.LAYOUT_PACKED, slabs[j])
                waits.append(c.get_option("key_writer_waits") - w0)
                c.encrypt_witness(dpt, None, out=outs[j - 1], want_ct=True)
        torch.cuda.synchronize()
        delay.assert_overlap(ev_b_before, ev_a_end, "schedule(k5) on B")
        with torch.cuda.stream(b):
            c.encrypt_witness(dpt, None, out=after[0], want_ct=True)
        with torch.cuda.stream(cs):
            c.encrypt_witness(dpt, None, out=after[1], want_ct=True)
        torch.cuda.synchronize()
        arena.check()
        for j, u in enumerate(us):
            _slab_is("key slab of schedule(%s)" % u.name, _snap(slabs[j], SLAB), u, us[:j] + us[j + 1:])
        for j in range(1, 5):
            _carries("launch behind schedule(%s) on B" % us[j].name, _snap(outs[j - 1], ENC), us[j], us[:j] + us[j + 1:])
        for where, w in zip(("B", "C"), after):
            _carries("launch on %s after a synchronise" % where, _snap(w, ENC), us[4], us[:4])
        assert waits == [0, 0, 0, 1], waits
        assert c.get_option("key_reader_waits") == r0
    finally:
        torch.cuda.synchronize()
        c.close()


def test_host_schedule_behind_a_pending_device_writer(pkg, oracle, delay):
    """key_slots = 1.  schedule(k1) on stream A, held by the delay; then the host entry point schedule_key_host(k2), which
    launches on the null stream and takes the one slot again; then encrypt_witness_host(pt, None) and a device launch on
    another stream.  All carry k2.  Whether the null stream runs beside A cannot be shown with an event recorded before the
    call (the entry point synchronises the device before it returns), so this case asserts the bytes and the statistics
    only: exactly one schedule waited for another stream's writer."""
    import torch
    rng = np.random.default_rng(4103)
    n = 4000
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    k1, k2 = _keys(rng, 2)
    u1, u2 = _Under(oracle, pt, "k1", k1), _Under(oracle, pt, "k2", k2)
    u2.witness()
    c = pkg.Context(0)
    harena = guarded.HostArena(guarded.CANARIES[1])
    try:
        c.set_option("key_slots", 1)
        arena = guarded.DeviceArena(guarded.CANARIES[0])
        dpt, dk1 = torch.from_numpy(pt).cuda(), torch.from_numpy(k1).cuda()
        slab1 = arena.key_witness(pkg, 1, pkg.LAYOUT_PACKED, want_rk=False)
        out_b = arena.witness(pkg, n, pkg.LAYOUT_PACKED, key_slab=False)
        hw = pkg.Witness(*[harena.out("xyz"[i], n * pkg.column_stride(pkg.LAYOUT_PACKED, i)) for i in range(3)],
                         harena.out("ct", n * 16, (n, 16)), None)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        w0 = c.get_option("key_writer_waits")
        delay.hold(a)
        with torch.cuda.stream(a):
            guarded.schedule_key(c, pkg, dk1, pkg.LAYOUT_PACKED, slab1)
        kw2 = c.schedule_key_host(k2)
        guarded.encrypt_witness_host(c, pkg, pt, None, n, pkg.LAYOUT_PACKED, hw)
        with torch.cuda.stream(b):
            c.encrypt_witness(dpt, None, out=out_b, want_ct=True)
        torch.cuda.synchronize()
        arena.check()
        harena.check()
        _slab_is("key slab of schedule(k1) on A", _snap(slab1, SLAB), u1, [u2])
        _slab_is("key slab of schedule_key_host(k2)", _snap(kw2, SLAB), u2, [u1])
        _carries("encrypt_witness_host behind schedule_key_host", _snap(hw, ENC), u2, [u1])
        _carries("device launch behind schedule_key_host", _snap(out_b, ENC), u2, [u1])
        assert c.get_option("key_writer_waits") - w0 == 1
    finally:
        torch.cuda.synchronize()
        c.close()
        harena.close()


def test_cached_arena_is_handed_out_only_behind_its_previous_launches(pkg, oracle, delay):
    """The placement cache.  Probed columns for n = 2^17 + 48 blocks with ciphertext and key slabs; a per-block-key launch
    into them under keys K1 on stream A, held by the delay; aesw_columns_free while that launch is still queued; the same
    shape again is a cache hit (no candidate built, the same column pointers).  Poisoned, then a launch under keys K2 on
    stream B, which runs beside A.  aesw_columns_free waits for outstanding device work, as hipFree does, so every column --
    x, y, z, ct and the four key-slab columns -- holds the oracle's bytes under K2, none of K1's."""
    import torch
    rng = np.random.default_rng(4105)
    n = (1 << 17) + 48
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    K1, K2 = _keys(rng, 2, n)
    u1, u2 = _Under(oracle, pt, "K1", K1), _Under(oracle, pt, "K2", K2)
    u2.witness()
    u2.slab()
    c = pkg.Context(0)
    views = {}  # the arena's device views live here only: dropped before the context (and its mappings) goes
    try:
        assert c.get_option("arena_cache") == 1
        dpt, dK1, dK2 = (torch.from_numpy(x).cuda() for x in (pt, K1, K2))

        def members(w):
            return [getattr(w, col) for col in ENC] + [getattr(w.key, col) for col in SLAB]

        views["first"] = c.alloc_columns(n, pkg.LAYOUT_PACKED, want_ct=True, key_slab=True)
        assert c.last_arena["candidates"] >= 1
        ptrs = [t.data_ptr() for t in members(views["first"])]
        a = torch.cuda.Stream()
        b = delay.free_stream(a)
        torch.cuda.synchronize()
        hits0 = c.get_option("arena_cache_hits")
        ev_a_end, ev_b_before = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        delay.hold(a)
        with torch.cuda.stream(a):
            c.encrypt_witness(dpt, dK1, out=views["first"], want_ct=True, key_slab=True)
        ev_a_end.record(a)
        ev_b_before.record(b)
        c.free_columns(views.pop("first"))
        views["again"] = c.alloc_columns(n, pkg.LAYOUT_PACKED, want_ct=True, key_slab=True)
        hit = (c.last_arena["candidates"], [t.data_ptr() for t in members(views["again"])], c.get_option("arena_cache_hits") - hits0)
        with torch.cuda.stream(b):
            for t in members(views["again"]):
                t.fill_(guarded.CANARIES[0])
            del t
            c.encrypt_witness(dpt, dK2, out=views["again"], want_ct=True, key_slab=True)
        torch.cuda.synchronize()
        got, got_key = _snap(views["again"], ENC), _snap(views["again"].key, SLAB)
        c.free_columns(views.pop("again"))
        assert hit == (0, ptrs, 1), "not a cache hit: %r" % (hit,)
        delay.assert_overlap(ev_b_before, ev_a_end, "free, alloc and launch on B")
        _carries("launch into the cached arena", got, u2, [u1])
        _slab_is("key slabs in the cached arena", got_key, u2, [u1])
    finally:
        views.clear()
        torch.cuda.synchronize()
        c.close()
