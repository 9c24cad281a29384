"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle.

Bit-exact is the bar: this is byte/integer work.  Small and medium sizes are
compared byte-for-byte with the oracle; BASELINE.json's full sizes use
size-independent properties (see test_gpu_full_size.py).
"""
import numpy as np
import pytest

import guarded
import oracle_lib as ol

pytestmark = pytest.mark.gpu

SEED = 0xA35128


def _inputs(n, seed=SEED, force_ff=True):
    rng = np.random.default_rng(seed)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if force_ff and n > 1:
        pt[1] = 0xFF
        keys[1] = 0  # pt ^ key == 0xff -> S_BOX[255], the reference's non-FIPS entry
    return pt, keys


def _cmp(name, got, exp):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if not np.array_equal(got.reshape(-1), exp.reshape(-1)):
        bad = np.nonzero(got.reshape(-1) != exp.reshape(-1))[0]
        raise AssertionError("%s: %d bytes differ, first at %d (got %d exp %d)" %
                             (name, bad.size, bad[0], got.reshape(-1)[bad[0]], exp.reshape(-1)[bad[0]]))


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED, ol.VALUES])
@pytest.mark.parametrize("n", [1, 3, 16, 17, 63, 64, 65, 1000])
def test_shared_key_small(ctx, oracle, layout, n):
    import torch
    pt, keys = _inputs(n)
    got = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys[0]).cuda(), layout=layout,
                              want_ct=True, key_slab=True)
    torch.cuda.synchronize()
    exp = oracle.encrypt_witness(pt, keys[0], layout=layout)
    for c in "xyz":
        _cmp(c, getattr(got, c), getattr(exp, c))
    _cmp("ct", got.ct, exp.ct)
    kexp = oracle.key_schedule_witness(keys[0], layout=layout)
    for c in ("w", "kx", "ky", "kz"):
        _cmp(c, getattr(got.key, c), getattr(kexp, c))


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED, ol.VALUES])
@pytest.mark.parametrize("n", [1, 5, 16, 33, 64, 257, 1000])
def test_per_block_keys_small(ctx, oracle, layout, n):
    import torch
    pt, keys = _inputs(n)
    got = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda(), layout=layout,
                              want_ct=True, key_slab=True)
    torch.cuda.synchronize()
    exp = oracle.encrypt_witness(pt, keys, layout=layout)
    for c in "xyz":
        _cmp(c, getattr(got, c), getattr(exp, c))
    _cmp("ct", got.ct, exp.ct)
    kexp = oracle.key_schedule_witness(keys, layout=layout)
    for c in ("w", "kx", "ky", "kz"):
        _cmp(c, getattr(got.key, c), getattr(kexp, c))


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED, ol.VALUES])
def test_per_block_keys_without_key_slab(ctx, oracle, layout):
    import torch
    pt, keys = _inputs(200)
    got = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda(), layout=layout, want_ct=True)
    torch.cuda.synchronize()
    exp = oracle.encrypt_witness(pt, keys, layout=layout)
    for c in "xyz":
        _cmp(c, getattr(got, c), getattr(exp, c))
    _cmp("ct", got.ct, exp.ct)


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED])
@pytest.mark.parametrize("n", [1, 15, 16, 100])
def test_key_schedule_kernel(ctx, pkg, oracle, layout, n):
    _, keys = _inputs(n)
    exp = oracle.key_schedule_witness(keys, layout=layout)
    try:
        for i, mode in enumerate((1, 0, 2)):  # nontemporal (default), plain, write-through
            ctx.set_option("key_store_mode", mode)
            # every mode writes into its own poisoned, guard-banded outputs: none can pass on the previous mode's bytes
            a = guarded.DeviceArena(guarded.CANARIES[i % 2])
            got = a.key_witness(pkg, n, layout, want_rk=True)
            assert all(a.poisoned(t) for t in got)
            guarded.key_schedule(ctx, a.input("keys", keys), layout, got)
            a.check()
            for c in ("w", "kx", "ky", "kz", "rk"):
                _cmp(c, getattr(got, c), getattr(exp, c))
    finally:
        ctx.set_option("key_store_mode", 1)


def test_zero_vector_and_fips_kats(ctx, oracle):
    """The reference's only vector (all-zero, src/aes128.rs:409-418) and FIPS-197
    App. B / C.1, which agree under both S-boxes (no 0xff reached)."""
    import torch
    cases = [
        ("00" * 16, "00" * 16, "66e94bd4ef8a2c3b884cfa59ca342b2e"),
        ("3243f6a8885a308d313198a2e0370734", "2b7e151628aed2a6abf7158809cf4f3c", "3925841d02dc09fbdc118597196a0b32"),
        ("00112233445566778899aabbccddeeff", "000102030405060708090a0b0c0d0e0f", "69c4e0d86a7b0430d8cdb78070b4c55a"),
    ]
    for pt_hex, key_hex, ct_hex in cases:
        pt = np.frombuffer(bytes.fromhex(pt_hex), np.uint8).reshape(1, 16).copy()
        key = np.frombuffer(bytes.fromhex(key_hex), np.uint8).copy()
        got = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(key).cuda(), layout=ol.DENSE, want_ct=True)
        torch.cuda.synchronize()
        assert got.ct.cpu().numpy().tobytes().hex() == ct_hex
        # the sbox rows never see 0xff here, which is why these KATs are valid for the reference's table
        x = got.x.cpu().numpy()
        sbox_rows = np.concatenate([np.arange(32 + 144 * r, 48 + 144 * r) for r in range(9)] + [np.arange(1328, 1344)])
        assert not np.any(x[sbox_rows] == 0xFF)


def test_sbox_ff_differs_from_fips(ctx, pkg, oracle):
    """pt^key == 0xff reaches S_BOX[255]: the reference table (23) and FIPS (22)
    must give different witnesses, and the device follows whatever the host passes."""
    import torch
    pt = np.full((1, 16), 0xFF, np.uint8)
    key = np.zeros(16, np.uint8)
    ref = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(key).cuda(), layout=ol.DENSE, want_ct=True)
    torch.cuda.synchronize()
    assert int(ref.y.cpu().numpy()[32]) == 23
    fctx = pkg.Context(0, tables=pkg.fips_tables())
    fips = fctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(key).cuda(), layout=ol.DENSE, want_ct=True)
    torch.cuda.synchronize()
    assert int(fips.y.cpu().numpy()[32]) == 22
    assert not np.array_equal(ref.ct.cpu().numpy(), fips.ct.cpu().numpy())
    # FIPS-197 ciphertext of (ff..ff, 00..00) from an independent AES implementation of the standard
    forc = ol.Oracle(tables=oracle.fips_tables())
    _cmp("fips ct", fips.ct, forc.encrypt_witness(pt, key, layout=ol.DENSE).ct)
    fctx.close()


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED, ol.VALUES])
def test_generic_table_path(ctx, pkg, oracle, layout):
    """Tables that are NOT xtime tables force the LDS-lookup MixColumns path;
    the device must follow them (the host's lookup table is the arbiter)."""
    import torch
    rng = np.random.default_rng(5)
    sbox = rng.permutation(256).astype(np.uint8)
    mul2 = rng.integers(0, 256, 256, dtype=np.uint8)
    mul3 = rng.integers(0, 256, 256, dtype=np.uint8)
    c2 = pkg.Context(0, tables=(sbox, mul2, mul3))
    assert not c2.uses_xtime_path and ctx.uses_xtime_path
    pt, keys = _inputs(130)
    o2 = ol.Oracle(tables=(sbox, mul2, mul3))
    for k_host in (keys[0], keys):
        got = c2.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(np.ascontiguousarray(k_host)).cuda(),
                                 layout=layout, want_ct=True, key_slab=True)
        torch.cuda.synchronize()
        exp = o2.encrypt_witness(pt, k_host, layout=layout)
        for c in "xyz":
            _cmp(c, getattr(got, c), getattr(exp, c))
        kexp = o2.key_schedule_witness(k_host, layout=layout)
        for c in ("w", "kx", "ky", "kz"):
            _cmp(c, getattr(got.key, c), getattr(kexp, c))
    # same real tables through the generic path == through the xtime path
    c3 = pkg.Context(0)
    c3.set_option("force_table_path", 1)
    assert not c3.uses_xtime_path
    a = c3.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda(), layout=layout)
    b = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys).cuda(), layout=layout)
    torch.cuda.synchronize()
    for c in "xyz":
        assert torch.equal(getattr(a, c), getattr(b, c))
    c2.close()
    c3.close()


@pytest.mark.parametrize("waves", [1, 2, 3, 4])
@pytest.mark.parametrize("nt", [0, 1, 2])
def test_launch_options(pkg, oracle, waves, nt):
    import torch
    c = pkg.Context(0)
    c.set_option("waves_shared", waves)
    c.set_option("waves_pbk", waves)
    c.set_option("store_mode", nt)
    pt, keys = _inputs(300)
    for layout in (ol.DENSE, ol.PACKED, ol.VALUES):
        for k_host in (keys[0], keys):
            a = guarded.DeviceArena(guarded.CANARIES[k_host.ndim - 1])  # poisoned: no case passes on the previous case's bytes
            out = a.witness(pkg, 300, layout, want_ct=False, key_slab=True, n_keys=1 if k_host.ndim == 1 else 300)
            got = c.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(np.ascontiguousarray(k_host)).cuda(),
                                    layout=layout, key_slab=True, out=out)
            a.check()
            exp = oracle.encrypt_witness(pt, k_host, layout=layout)
            for col in "xyz":
                _cmp(col, getattr(got, col), getattr(exp, col))
            kexp = oracle.key_schedule_witness(k_host, layout=layout)
            for col in ("w", "kx", "ky", "kz"):
                _cmp(col, getattr(got.key, col), getattr(kexp, col))
    c.close()


@pytest.mark.parametrize("layout", [ol.DENSE, ol.PACKED, ol.VALUES])
def test_schedule_key_then_encrypt(pkg, oracle, layout):
    """The reference's call shape: schedule_key() once, encrypt() n times
    (benches/aes128.rs:50-53); encrypt before schedule_key fails like the
    reference's expect("Keys should be scheduled") (src/aes128.rs:170)."""
    import torch
    c = pkg.Context(0)
    pt, keys = _inputs(333)
    dpt = torch.from_numpy(pt).cuda()
    with pytest.raises(pkg.AeswError) as e:
        c.encrypt_witness(dpt, None, layout=layout)
    assert e.value.status == 6
    kw = c.schedule_key(torch.from_numpy(keys[7]).cuda(), layout=layout)
    got = c.encrypt_witness(dpt, None, layout=layout, want_ct=True)
    torch.cuda.synchronize()
    exp = oracle.encrypt_witness(pt, keys[7], layout=layout)
    for col in "xyz":
        _cmp(col, getattr(got, col), getattr(exp, col))
    _cmp("ct", got.ct, exp.ct)
    kexp = oracle.key_schedule_witness(keys[7], layout=layout)
    for col in ("w", "kx", "ky", "kz"):
        _cmp(col, getattr(kw, col), getattr(kexp, col))
    # a new key replaces the old one
    c.schedule_key(torch.from_numpy(keys[8]).cuda(), layout=layout, key_slab=False)
    got = c.encrypt_witness(dpt, None, layout=layout)
    torch.cuda.synchronize()
    _cmp("x", got.x, oracle.encrypt_witness(pt, keys[8], layout=layout).x)
    c.close()


@pytest.mark.parametrize("remap", [0, 1])
def test_xcd_remap(pkg, oracle, remap):
    """xcd_remap (default on) only permutes which workgroup takes which block group (any group count, incl. non-multiples of 8)."""
    import torch
    c = pkg.Context(0)
    assert c.get_option("xcd_remap") == 1
    c.set_option("xcd_remap", remap)
    for n in (64 * 11 + 5, 64 * 8, 37):
        pt, keys = _inputs(n)
        for k_host in (keys[0], keys):
            a = guarded.DeviceArena(guarded.CANARIES[remap])  # poisoned: the other remap's bytes cannot be inherited
            out = a.witness(pkg, n, ol.PACKED, want_ct=True, key_slab=False)
            got = c.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(np.ascontiguousarray(k_host)).cuda(),
                                    layout=ol.PACKED, want_ct=True, out=out)
            a.check()
            exp = oracle.encrypt_witness(pt, k_host, layout=ol.PACKED)
            for col in "xyz":
                _cmp(col, getattr(got, col), getattr(exp, col))
            _cmp("ct", got.ct, exp.ct)
    c.close()


@pytest.mark.parametrize("cap", [1, 3, 8, 16, 512])
def test_group_striding(pkg, oracle, cap):
    """grid_cap < number of block groups: every workgroup walks several groups, reusing its LDS windows."""
    import torch
    c = pkg.Context(0)
    c.set_option("grid_cap", cap)
    pt, keys = _inputs(1111)
    for layout in (ol.DENSE, ol.PACKED, ol.VALUES):
        for k_host in (keys[0], keys):
            a = guarded.DeviceArena(guarded.CANARIES[cap % 2])  # poisoned: the previous cap's bytes cannot be inherited
            out = a.witness(pkg, 1111, layout, want_ct=True, key_slab=True, n_keys=1 if k_host.ndim == 1 else 1111)
            got = c.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(np.ascontiguousarray(k_host)).cuda(),
                                    layout=layout, want_ct=True, key_slab=True, out=out)
            a.check()
            exp = oracle.encrypt_witness(pt, k_host, layout=layout)
            for col in "xyz":
                _cmp(col, getattr(got, col), getattr(exp, col))
            _cmp("ct", got.ct, exp.ct)
            kexp = oracle.key_schedule_witness(k_host, layout=layout)
            for col in ("w", "kx", "ky", "kz"):
                _cmp(col, getattr(got.key, col), getattr(kexp, col))
    c.close()


def test_unaligned_column_buffers(ctx, oracle):
    """Column pointers need only 16-byte alignment (128 is just faster)."""
    import torch
    import halo2_aes_amd as pkg
    for n in (200, 37, 1):
        pt, keys = _inputs(n)
        for layout in (ol.DENSE, ol.PACKED, ol.VALUES):
            strides = ol.ENC_STRIDE[layout]
            bufs = [torch.full((n * s + 4096,), 0xCD, dtype=torch.uint8, device="cuda") for s in strides]
            offs = (16, 48, 112)
            out = pkg.Witness(*[b[o:o + n * s] for b, o, s in zip(bufs, offs, strides)], None, None)
            ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(keys[0]).cuda(), layout=layout, out=out)
            torch.cuda.synchronize()
            exp = oracle.encrypt_witness(pt, keys[0], layout=layout)
            for b, o, s, name in zip(bufs, offs, strides, "xyz"):
                h = b.cpu().numpy()
                assert np.array_equal(h[o:o + n * s], getattr(exp, name)), name
                assert np.all(h[:o] == 0xCD) and np.all(h[o + n * s:] == 0xCD), "wrote outside the column buffer"


def test_config1_single_block(ctx):
    """BASELINE config 0: one block, fixed zero key (benches/aes128.rs shape)."""
    import torch
    got = ctx.encrypt_witness(torch.zeros((1, 16), dtype=torch.uint8, device="cuda"),
                              torch.zeros(16, dtype=torch.uint8, device="cuda"), layout=ol.DENSE, want_ct=True)
    torch.cuda.synchronize()
    assert got.ct.cpu().numpy().tobytes().hex() == "66e94bd4ef8a2c3b884cfa59ca342b2e"


def test_config2_2p16_shared_key_bit_exact(ctx, oracle):
    """BASELINE config 1: 2^16 blocks, one shared random key, every advice byte
    compared with the oracle (both layouts)."""
    import torch
    n = 1 << 16
    rng = np.random.default_rng(SEED + 1)
    pt = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    key = rng.integers(0, 256, 16, dtype=np.uint8)
    dpt, dkey = torch.from_numpy(pt).cuda(), torch.from_numpy(key).cuda()
    for layout in (ol.DENSE, ol.PACKED):
        got = ctx.encrypt_witness(dpt, dkey, layout=layout, want_ct=True)
        torch.cuda.synchronize()
        exp = oracle.encrypt_witness(pt, key, layout=layout, threads=16)
        for c in "xyz":
            _cmp(c, getattr(got, c), getattr(exp, c))
        _cmp("ct", got.ct, exp.ct)


def test_lookup_table(ctx, oracle):
    import torch
    t = ctx.lookup_table()
    torch.cuda.synchronize()
    _cmp("table", t, oracle.lookup_table())


def test_expand_fr(ctx):
    """Byte -> bn256::Fr Montgomery cell (Fp::from(u64)): v * 2^256 mod r, little-endian."""
    import torch
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    cells = torch.arange(0, 256, dtype=torch.uint8, device="cuda").repeat(5)
    out = ctx.expand_fr(cells)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for i in (0, 1, 2, 17, 255, 256, 700, 1279):
        v = i % 256
        assert int.from_bytes(out[i].tobytes(), "little") == (v << 256) % r
    # halo2curves bn256::Fr::one() limbs (R = 2^256 mod r)
    assert out[1].tobytes() == bytes.fromhex("fbffff4f1c3496ac29cd609f9576fc362e4679786fa36e662fdf079ac1770a0e")


def test_host_pointer_path(ctx, oracle):
    """aesw_encrypt_witness (host buffers, chunked + overlapped D2H)."""
    pt, keys = _inputs(5000)
    ctx.set_option("chunk_blocks", 1024)  # force several pipeline stages
    try:
        for layout in (ol.DENSE, ol.PACKED, ol.VALUES):
            for k_host in (keys[0], keys):
                got = ctx.encrypt_witness_host(pt, k_host, layout=layout, want_ct=True, key_slab=True)
                exp = oracle.encrypt_witness(pt, k_host, layout=layout)
                for c in "xyz":
                    _cmp(c, getattr(got, c), getattr(exp, c))
                _cmp("ct", got.ct, exp.ct)
                kexp = oracle.key_schedule_witness(k_host, layout=layout)
                for c in ("w", "kx", "ky", "kz"):
                    _cmp(c, getattr(got.key, c), getattr(kexp, c))
        kw = ctx.key_schedule_witness_host(keys[:77], layout=ol.PACKED)
        kexp = oracle.key_schedule_witness(keys[:77], layout=ol.PACKED)
        for c in ("w", "kx", "ky", "kz", "rk"):
            _cmp(c, getattr(kw, c), getattr(kexp, c))
        _cmp("table", ctx.lookup_table_host(), oracle.lookup_table())
    finally:
        ctx.set_option("chunk_blocks", 1 << 15)


def test_host_pointer_path_pinned_outputs(ctx, pkg, oracle):
    """Page-locked caller buffers (aesw_host_alloc) take the direct-DMA branch."""
    pt, keys = _inputs(3000)
    ctx.set_option("chunk_blocks", 1024)
    outs = [pkg.api.host_alloc(3000 * pkg.column_stride(ol.PACKED, c)) for c in range(3)]
    try:
        import torch
        ctx.schedule_key(torch.from_numpy(keys[0]).cuda(), layout=ol.PACKED, key_slab=False)
        torch.cuda.synchronize()
        got = ctx.encrypt_witness_host(pt, None, layout=ol.PACKED, out_cols=outs)
        exp = oracle.encrypt_witness(pt, keys[0], layout=ol.PACKED)
        for c in "xyz":
            _cmp(c, getattr(got, c), getattr(exp, c))
    finally:
        for o in outs:
            pkg.api.host_free(o)
        ctx.set_option("chunk_blocks", 1 << 15)


def test_streaming_host_path(ctx, pkg, oracle):
    """aesw_encrypt_witness_stream (BASELINE configs[4] shape): chunks arrive in order while the next is in flight."""
    import torch
    pt, keys = _inputs(5000)
    ctx.set_option("chunk_blocks", 1024)
    try:
        for layout in (ol.DENSE, ol.PACKED, ol.VALUES):
            strides = ol.ENC_STRIDE[layout]
            for k_host in (None, keys[3], keys):
                if k_host is None:
                    ctx.schedule_key(torch.from_numpy(keys[3]).cuda(), layout=layout, key_slab=False)
                    torch.cuda.synchronize()
                got = [np.zeros(5000 * s, np.uint8) for s in strides]
                seen = []

                def consume(first, count, x, y, z):
                    seen.append((first, count))
                    for dst, src, s in zip(got, (x, y, z), strides):
                        dst[first * s:(first + count) * s] = src
                    return 0

                ctx.encrypt_witness_stream(pt, k_host, consume, layout=layout)
                assert seen == [(i, min(1024, 5000 - i)) for i in range(0, 5000, 1024)]
                exp = oracle.encrypt_witness(pt, keys[3] if k_host is None else k_host, layout=layout)
                for c, g in zip("xyz", got):
                    _cmp(c, g, getattr(exp, c))
        # the consumer can abort the stream
        with pytest.raises(pkg.AeswError) as e:
            ctx.encrypt_witness_stream(pt, keys[3], lambda *a: 1, layout=ol.PACKED)
        assert e.value.status == 7
    finally:
        ctx.set_option("chunk_blocks", 1 << 15)


def test_argument_errors(ctx, pkg):
    import torch
    pt = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ctx.encrypt_witness(pt, torch.zeros((3, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        ctx.encrypt_witness(pt.cpu(), torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(pkg.AeswError):
        ctx.set_option("no_such_option", 1)
    # misaligned column buffer -> AESW_ERR_INVALID_ARG from the C ABI
    w = ctx.alloc_witness(4, ol.DENSE)
    big = torch.empty(4 * 1360 + 16, dtype=torch.uint8, device="cuda")
    bad = pkg.Witness(big[1:], w.y, w.z, None, None)
    with pytest.raises(pkg.AeswError) as e:
        ctx.encrypt_witness(pt, torch.zeros(16, dtype=torch.uint8, device="cuda"), layout=ol.DENSE, out=bad)
    assert e.value.status == 1
    # empty batch is a no-op
    out = ctx.encrypt_witness(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"),
                              torch.zeros(16, dtype=torch.uint8, device="cuda"))
    assert out.x.numel() == 0


def test_structured_inputs(ctx, oracle):
    """Non-random inputs: every byte value repeated, counters, all-ones, pt == key, pt == ~key."""
    import torch
    cases = []
    v = np.arange(256, dtype=np.uint8)
    cases.append((np.repeat(v, 16).reshape(256, 16), np.repeat(v[::-1], 16).reshape(256, 16)))
    cases.append((np.arange(256 * 16, dtype=np.uint32).astype(np.uint8).reshape(256, 16), np.zeros((256, 16), np.uint8)))
    cases.append((np.full((64, 16), 0xFF, np.uint8), np.full((64, 16), 0xFF, np.uint8)))
    k = np.random.default_rng(8).integers(0, 256, (128, 16), dtype=np.uint8)
    cases.append((k.copy(), k))           # first sbox input 0 everywhere
    cases.append((k ^ 0xFF, k))           # first sbox input 0xff everywhere (the reference's S_BOX[255])
    for pt, keys in cases:
        for layout in (ol.DENSE, ol.PACKED):
            got = ctx.encrypt_witness(torch.from_numpy(pt).cuda(), torch.from_numpy(np.ascontiguousarray(keys)).cuda(),
                                      layout=layout, want_ct=True, key_slab=True)
            torch.cuda.synchronize()
            exp = oracle.encrypt_witness(pt, keys, layout=layout)
            for c in "xyz":
                _cmp(c, getattr(got, c), getattr(exp, c))
            _cmp("ct", got.ct, exp.ct)
            kexp = oracle.key_schedule_witness(keys, layout=layout)
            for c in ("w", "kx", "ky", "kz"):
                _cmp(c, getattr(got.key, c), getattr(kexp, c))


def test_two_contexts_two_threads(pkg, oracle):
    """Contexts are thread-compatible: two host threads, each with its own context and stream, at once."""
    import threading
    import torch
    pt, keys = _inputs(20000)
    results, errors = {}, []

    def work(idx, layout):
        try:
            c = pkg.Context(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dpt = torch.from_numpy(pt).cuda()
                for _ in range(5):
                    got = c.encrypt_witness(dpt, torch.from_numpy(keys[idx]).cuda(), layout=layout, want_ct=True)
                stream.synchronize()
                results[idx] = (layout, got.x.cpu().numpy(), got.y.cpu().numpy(), got.z.cpu().numpy())
            c.close()
        except Exception as e:  # surfaced in the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i, l)) for i, l in ((0, ol.DENSE), (1, ol.PACKED))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for idx, (layout, x, y, z) in results.items():
        exp = oracle.encrypt_witness(pt, keys[idx], layout=layout)
        _cmp("x", x, exp.x); _cmp("y", y, exp.y); _cmp("z", z, exp.z)


def test_plain_c_host(pkg, tmp_path):
    """The C ABI from a plain C program (gcc, no Python/torch in the process): examples/aesw_demo.c."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "aesw_demo"
    lib_dir = root / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-I", str(root / "include"), str(root / "examples" / "aesw_demo.c"),
                    "-o", str(exe), "-L", str(lib_dir), "-laesw", "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"],
                   check=True)
    out = subprocess.run([str(exe), "20000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "66e94bd4ef8a2c3b884cfa59ca342b2e" in out.stdout and "ok" in out.stdout


def test_end_to_end_example(pkg):
    """examples/end_to_end.py: device witness -> synthesize() + MockProver -> values-only -> Fr columns -> keygen data."""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("aesw_end_to_end", Path(__file__).resolve().parent.parent / "examples" / "end_to_end.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(n=150, k=16, n_sets=4)


def test_committed_golden_fixtures(ctx):
    """The HIP path against tests/golden/slab_vectors.npz directly (no oracle in the loop): the reference's
    zero vector, FIPS-197 App. B / C.1, the S_BOX[0xff] block and seeded random blocks, both layouts,
    per-block keys with key witness and one shared key."""
    import torch
    from pathlib import Path
    g = np.load(Path(__file__).resolve().parent / "golden" / "slab_vectors.npz")
    dpt, dkeys = torch.from_numpy(g["pt"]).cuda(), torch.from_numpy(g["keys"]).cuda()
    for layout, name in ((ol.DENSE, "dense"), (ol.PACKED, "packed"), (ol.VALUES, "values")):
        got = ctx.encrypt_witness(dpt, dkeys, layout=layout, want_ct=True, key_slab=True)
        shared = ctx.encrypt_witness(dpt, dkeys[4].contiguous(), layout=layout)
        kw = ctx.key_schedule_witness(dkeys, layout=layout)
        torch.cuda.synchronize()
        for c in "xyz":
            _cmp(name + " " + c, getattr(got, c), g["%s_%s" % (name, c)])
            _cmp(name + " shared " + c, getattr(shared, c), g["%s_shared_%s" % (name, c)])
        _cmp(name + " ct", got.ct, g["%s_ct" % name])
        for c in ("w", "kx", "ky", "kz"):
            _cmp(name + " " + c, getattr(got.key, c), g["%s_%s" % (name, c)])
        _cmp(name + " rk", kw.rk, g["%s_rk" % name])
    assert got.ct[0].cpu().numpy().tobytes().hex() == "66e94bd4ef8a2c3b884cfa59ca342b2e"
