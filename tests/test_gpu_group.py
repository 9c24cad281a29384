"""Device groups on the GPU (include/aesw.h "device groups"): one aesw_ctx over several member contexts, driven from one process.
On a one-GPU machine the members share device 0 ([0, 0], [0, 0, 0]): the sharding, the threads, the offsets into the caller's
buffers and the stream hand-over are the same code whatever device a member drives.  Every group result is held to a plain
Context(0) run of the same batch, byte for byte, and sampled blocks to the CPU oracle."""
import ctypes as C
import subprocess
import threading
import time
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N = (1 << 16) + 5
GROUPS = [[0, 0], [0, 0, 0]]
ERR_INVALID_ARG, ERR_MISMATCH = 1, 7


def _batch(seed, n=N, pbk=True):
    rng = np.random.default_rng(seed)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16) if pbk else 16, dtype=np.uint8)
    return pt, keys


def _same(a, b, what):
    for name in ("x", "y", "z", "ct"):
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None) == (v is None), (what, name)
        if u is not None:
            assert np.array_equal(u, v), "%s: column %s differs" % (what, name)
    assert (a.key is None) == (b.key is None), what
    if a.key is not None:
        for name in ("w", "kx", "ky", "kz"):
            assert np.array_equal(getattr(a.key, name), getattr(b.key, name)), "%s: key slab %s differs" % (what, name)


def _samples(g, n):
    """Blocks on both sides of every shard boundary, the ends, and a few in between."""
    s = {0, n - 1, n // 2}
    for i in range(g.size):
        first, count = g.shard(n, i)
        s.update(b for b in (first - 1, first, first + 1, first + count - 1) if 0 <= b < n)
    return sorted(s)


def _check_oracle(oracle, pt, keys, got, layout, blocks):
    pbk = keys.size != 16
    idx = np.array(blocks)
    e = oracle.encrypt_witness(pt[idx], keys[idx] if pbk else keys, layout=layout)
    for c, name in enumerate("xyz"):
        s = pkg_stride(layout, c)
        if s == 0:
            continue
        g = getattr(got, name).reshape(-1, s)[idx]
        assert np.array_equal(g.reshape(-1), getattr(e, name)), "oracle: column %s" % name
    if got.ct is not None:
        assert np.array_equal(got.ct[idx], e.ct)


def pkg_stride(layout, c):
    return ol.ENC_STRIDE[layout][c]


@pytest.mark.parametrize("devices", GROUPS, ids=["g2", "g3"])
@pytest.mark.parametrize("layout", [ol.PACKED, ol.DENSE, ol.VALUES], ids=["packed", "dense", "values"])
def test_host_path_per_block_keys_equals_one_context(pkg, oracle, devices, layout):
    """Per-block keys with key slabs and ciphertext into pageable buffers: the group's bytes are the plain context's bytes."""
    pt, keys = _batch(11 + layout)
    plain = pkg.Context(0)
    want = plain.encrypt_witness_host(pt, keys, layout=layout, want_ct=True, key_slab=True)
    plain.close()
    g = pkg.Group(devices)
    assert g.size == len(devices) and g.device == 0
    got = g.encrypt_witness_host(pt, keys, layout=layout, want_ct=True, key_slab=True)
    _same(got, want, "group %r layout %d" % (devices, layout))
    _check_oracle(oracle, pt, keys, got, layout, _samples(g, N))
    kexp = oracle.key_schedule_witness(keys[_samples(g, N)], layout=layout)
    kl = ol.PACKED if layout == ol.VALUES else layout
    idx = np.array(_samples(g, N))
    for c, name in enumerate(("kx", "ky", "kz")):
        s = ol.KEY_STRIDE[kl][c]
        assert np.array_equal(getattr(got.key, name).reshape(-1, s)[idx].reshape(-1), getattr(kexp, name)), name
    assert np.array_equal(got.key.w.reshape(-1, 96)[idx].reshape(-1), kexp.w)
    g.close()


@pytest.mark.parametrize("devices", GROUPS, ids=["g2", "g3"])
def test_shared_and_scheduled_key_with_slab(pkg, oracle, devices):
    """One shared 16-byte key (its one key slab written once), and a key scheduled through the group (its slab from
    schedule_key_host, then encrypt with keys=None on every member)."""
    pt, key = _batch(23, pbk=False)
    plain = pkg.Context(0)
    want = plain.encrypt_witness_host(pt, key, layout=ol.PACKED, want_ct=True, key_slab=True)
    g = pkg.Group(devices)
    got = g.encrypt_witness_host(pt, key, layout=ol.PACKED, want_ct=True, key_slab=True)
    _same(got, want, "shared key")
    _check_oracle(oracle, pt, key, got, ol.PACKED, _samples(g, N))
    kexp = oracle.key_schedule_witness(key, layout=ol.PACKED)
    for name in ("w", "kx", "ky", "kz"):
        assert np.array_equal(getattr(got.key, name), getattr(kexp, name)), name
    # scheduled through the group
    key2 = np.arange(16, dtype=np.uint8) * 7
    slab = g.schedule_key_host(key2, layout=ol.PACKED)
    pslab = plain.schedule_key_host(key2, layout=ol.PACKED)
    kexp2 = oracle.key_schedule_witness(key2, layout=ol.PACKED)
    for name in ("w", "kx", "ky", "kz"):
        assert np.array_equal(getattr(slab, name), getattr(kexp2, name)), name
        assert np.array_equal(getattr(slab, name), getattr(pslab, name)), name
    got2 = g.encrypt_witness_host(pt, None, layout=ol.PACKED, want_ct=True)
    want2 = plain.encrypt_witness_host(pt, None, layout=ol.PACKED, want_ct=True)
    _same(got2, want2, "scheduled key")
    _check_oracle(oracle, pt, key2, got2, ol.PACKED, _samples(g, N))
    plain.close()
    g.close()


def test_page_locked_destinations(pkg):
    """aesw_host_alloc columns (direct DMA from every member) and pageable ones in one call."""
    pt, keys = _batch(31)
    plain = pkg.Context(0)
    want = plain.encrypt_witness_host(pt, keys, layout=ol.PACKED, want_ct=True, key_slab=True)
    plain.close()
    g = pkg.Group([0, 0])
    cols = [pkg.api.host_alloc(N * pkg_stride(ol.PACKED, c)) for c in range(3)]
    try:
        for c in cols:
            c[:] = 0xEE
        got = g.encrypt_witness_host(pt, keys, layout=ol.PACKED, want_ct=True, key_slab=True, out_cols=cols)
        _same(got, want, "page-locked columns")
    finally:
        for c in cols:
            pkg.api.host_free(c)
    g.close()


def test_more_members_than_blocks(pkg, oracle):
    """n = 2 over three members: the member with no blocks does nothing, the other two write their block; a shared key's slab
    is still written (by the first member with blocks)."""
    pt, keys = _batch(41, n=2)
    g = pkg.Group([0, 0, 0])
    assert [g.shard(2, i) for i in range(3)] == [(0, 0), (0, 1), (1, 1)]
    for k in (keys, keys[0]):
        plain = pkg.Context(0)
        want = plain.encrypt_witness_host(pt, k, layout=ol.PACKED, want_ct=True, key_slab=True)
        plain.close()
        got = g.encrypt_witness_host(pt, k, layout=ol.PACKED, want_ct=True, key_slab=True)
        _same(got, want, "n=2, %s key" % ("per-block" if k.size != 16 else "shared"))
        _check_oracle(oracle, pt, k, got, ol.PACKED, [0, 1])
    g.close()


def _stream(g, pt, keys, layout, on_chunk=None):
    n = pt.shape[0]
    strides = [pkg_stride(layout, c) for c in range(3)]
    out = [np.zeros(n * s, np.uint8) for s in strides]
    seen = np.zeros(n, np.int32)
    chunks, threads = [], set()

    def consume(first, count, x, y, z):
        threads.add(threading.get_ident())
        chunks.append((first, count))
        seen[first:first + count] += 1
        for o, src, s in zip(out, (x, y, z), strides):
            if s:
                o[first * s:(first + count) * s] = src
        return on_chunk(len(chunks)) if on_chunk else 0

    g.encrypt_witness_stream(pt, keys, consume, layout=layout)
    return out, seen, chunks, threads


@pytest.mark.parametrize("devices", GROUPS, ids=["g2", "g3"])
def test_stream_every_block_once_on_the_callers_thread(pkg, devices):
    pt, keys = _batch(51)
    g = pkg.Group(devices)
    g.set_option("chunk_blocks", 4096)
    g.set_option("stream_check", 1)
    want = g.encrypt_witness_host(pt, keys, layout=ol.PACKED)
    out, seen, chunks, threads = _stream(g, pt, keys, ol.PACKED)
    assert threads == {threading.get_ident()}  # consume runs on the calling thread only
    assert (seen == 1).all()  # every block exactly once
    for i in range(g.size):  # within a member: ascending, contiguous, covering its shard
        first, count = g.shard(N, i)
        mine = [c for c in chunks if first <= c[0] < first + count]
        assert mine == sorted(mine) and sum(c[1] for c in mine) == count
        assert mine[0][0] == first and all(a[0] + a[1] == b[0] for a, b in zip(mine, mine[1:]))
    for o, w, name in zip(out, (want.x, want.y, want.z), "xyz"):
        assert np.array_equal(o, w), "stream column %s" % name
    rep = g.last_stream_check()
    assert rep["blocks"] == N and rep["satisfied"] and rep["first"] is None, rep
    st = g.last_stream_stats()
    assert st["chunks"] == len(chunks) and st["bytes_to_host"] == N * sum(pkg_stride(ol.PACKED, c) for c in range(3))
    assert 0 < st["wall_ns"]
    g.close()


def test_stream_check_first_is_batch_wide(pkg):
    """A poisoned block in member 2's shard: the summed report names it by its batch-wide index."""
    pt, keys = _batch(53)
    g = pkg.Group([0, 0, 0])
    g.set_option("chunk_blocks", 4096)
    g.set_option("stream_check", 1)
    first, count = g.shard(N, 2)
    bad = first + count // 3
    # each member poisons its own block index + 1: only member 2's shard holds a block at bad - first
    for i in range(3):
        C_ = pkg.api.load_library()
        assert C_.aesw_set_option(g.member_handle(i), b"stream_poison", bad - first + 1 if i == 2 else 0) == 0
    _stream(g, pt, keys, ol.PACKED)
    rep = g.last_stream_check()
    assert not rep["satisfied"] and rep["first"][0] == bad and not rep["first"][1], (rep, bad)
    g.close()


def test_stream_abort_and_next_call(pkg):
    """consume returns 1 at its third chunk: AESW_ERR_MISMATCH once every member has stopped; the group is usable after."""
    pt, keys = _batch(61)
    g = pkg.Group([0, 0, 0])
    g.set_option("chunk_blocks", 4096)
    t0 = time.monotonic()
    with pytest.raises(pkg.AeswError) as e:
        _stream(g, pt, keys, ol.PACKED, on_chunk=lambda k: 1 if k == 3 else 0)
    assert e.value.status == ERR_MISMATCH
    assert time.monotonic() - t0 < 60
    assert g.last_stream_stats()["chunks"] < (N + 4095) // 4096
    want = pkg.Context(0).encrypt_witness_host(pt, keys, layout=ol.PACKED, want_ct=True, key_slab=True)
    got = g.encrypt_witness_host(pt, keys, layout=ol.PACKED, want_ct=True, key_slab=True)
    _same(got, want, "after an aborted stream")
    out, seen, _, _ = _stream(g, pt, keys, ol.PACKED)
    assert (seen == 1).all() and all(np.array_equal(o, w) for o, w in zip(out, (want.x, want.y, want.z)))
    g.close()


@pytest.mark.parametrize("pbk", [True, False], ids=["per-block", "shared"])
def test_check_witness_first_is_batch_wide(pkg, pbk):
    pt, keys = _batch(71, pbk=pbk)
    g = pkg.Group([0, 0, 0])
    w = g.encrypt_witness_host(pt, keys, layout=ol.PACKED, want_ct=True, key_slab=True)
    cols, kcols = [w.x, w.y, w.z], list(w.key[:4])
    rep = g.check_witness_host(pt, keys, cols, kcols, layout=ol.PACKED, ct=w.ct)
    assert rep["satisfied"] and rep["blocks"] == N and rep["keys"] == (N if pbk else 3), rep
    first, count = g.shard(N, 2)
    bad = first + count // 2
    z = w.z.copy()
    z[bad * 608 + 17] ^= 0x40
    rep = g.check_witness_host(pt, keys, [w.x, w.y, z], kcols, layout=ol.PACKED, ct=w.ct)
    assert not rep["satisfied"] and rep["first"][0] == bad and not rep["first"][1], (rep, bad)
    # the same bytes through one context report the same
    plain = pkg.Context(0)
    assert plain.check_witness_host(pt, keys, [w.x, w.y, z], kcols, layout=ol.PACKED, ct=w.ct)["first"] == rep["first"]
    plain.close()
    g.close()


def test_key_schedule_witness_host(pkg):
    rng = np.random.default_rng(81)
    keys = rng.integers(0, 256, (1001, 16), dtype=np.uint8)
    g = pkg.Group([0, 0, 0])
    plain = pkg.Context(0)
    a, b = g.key_schedule_witness_host(keys), plain.key_schedule_witness_host(keys)
    for name in ("w", "kx", "ky", "kz", "rk"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(g.lookup_table_host(), plain.lookup_table_host())
    plain.close()
    g.close()


def test_options_on_every_member_and_device_calls_refused(pkg):
    import os
    lib = pkg.api.load_library()
    g = pkg.Group([0, 0, 0])
    g.set_option("chunk_blocks", 12345)
    g.set_option("copy_threads", 3)
    v = C.c_int64()
    for i in range(3):
        h = g.member_handle(i)
        assert lib.aesw_get_option(h, b"chunk_blocks", C.byref(v)) == 0 and v.value == 12345
        assert lib.aesw_get_option(h, b"copy_threads", C.byref(v)) == 0 and v.value == 3
        assert lib.aesw_device(h) == 0
    assert g.get_option("chunk_blocks") == 12345
    with pytest.raises(IndexError):
        g.member_handle(3)
    g.set_option("copy_threads", -1)  # automatic: a quarter of the usable CPUs shared among three members
    usable = len(os.sched_getaffinity(0))
    assert g.get_option("effective_copy_threads") == max(1, min(4, usable // 12))
    with pytest.raises(pkg.AeswError):
        g.set_option("no_such_option", 1)
    # every device-pointer entry point refuses a group before it looks at a pointer
    h = g._h
    p = C.c_void_p(0)
    refused = [
        lib.aesw_schedule_key_device(h, p, 1, None, None),
        lib.aesw_encrypt_witness_device(h, p, p, 1, 1, 1, p, p, p, p, None, None),
        lib.aesw_encrypt_witness_batches_device(h, None, 0, 1, 1, None),
        lib.aesw_key_schedule_witness_device(h, p, 1, 1, p, p, p, p, p, None),
        lib.aesw_lookup_table_device(h, p, p, p, p, None),
        lib.aesw_expand_fr_device(h, p, 1, p, None),
        lib.aesw_check_witness_device(h, p, p, 1, 1, 1, p, p, p, p, None, p, None),
        lib.aesw_assemble_advice_device(h, 10, 1, 1, 1, p, p, p, None, 0, p, None),
        lib.aesw_assemble_advice_host(h, 10, 1, 1, 1, p, p, p, None, 0, p),
        lib.aesw_assemble_advice_stream(h, 10, 1, 1, 1, p, p, p, None, 0, p, None),
    ]
    cols = pkg.api.Columns()
    refused.append(lib.aesw_columns_alloc(h, 1, 1, 0, 0, C.byref(cols)))
    comm = C.c_void_p()
    refused.append(lib.aesw_comm_create(h, 1, 0, None, C.byref(comm)))
    assert refused == [ERR_INVALID_ARG] * len(refused), refused
    assert "group" in lib.aesw_last_error(h).decode()
    with pytest.raises(pkg.AeswError):
        g.encrypt_witness(None, None)
    g.close()


def test_plain_c_example(pkg, tmp_path):
    """examples/aesw_group.c: a group over devices 0 0 from plain C, checked against one context."""
    exe = tmp_path / "aesw_group"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "examples" / "aesw_group.c"), "-o", str(exe),
                    "-L", str(lib_dir), "-laesw", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe), "-n", str(N), "0", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout
