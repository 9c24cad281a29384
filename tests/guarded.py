"""Poisoned, guard-banded buffers for kernel tests (a helper module, not a conftest).

Every output is a view into a larger buffer filled with a canary byte: GUARD bytes or more on each side, the view starting
16-byte aligned but not 128-byte aligned (the C ABI's minimum for columns is 16).  Inputs sit at a 4-byte offset (the ABI's
minimum for pt / keys).  A kernel that skips a write leaves the canary, one that writes past a view damages a guard, and
check() names the buffer and the offset of the first damaged byte.  Run a case under both CANARIES and an unwritten byte whose
true value equals one canary still fails under the other.

Where a Python wrapper allocates its own outputs (rk of key_schedule_witness, the slab of schedule_key, lookup_table, the ct /
key slab of encrypt_witness_host), the functions at the bottom call the C ABI directly through ctypes."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_lib as ol

GUARD = 4096
VIEW_OFFSET = 80      # buffer base (>= 256-aligned) + GUARD + 80: 16-aligned, not 128-aligned
INPUT_OFFSET = 4      # 4-aligned, not 16-aligned
CANARIES = (0xA5, 0x5A)


def first_diff(got, exp):
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    if got.shape != exp.shape:
        return "size %d != %d" % (got.size, exp.size)
    bad = np.nonzero(got != exp)[0]
    if not bad.size:
        return None
    return "%d bytes differ, first at %d (got 0x%02x exp 0x%02x)" % (bad.size, bad[0], got[bad[0]], exp[bad[0]])


def assert_bytes(name, got, exp):
    d = first_diff(got, exp)
    if d:
        raise AssertionError("%s: %s" % (name, d))


class _Base:
    def __init__(self, canary: int):
        self.canary = canary
        self._bufs = {}  # name -> (backing, lo, nbytes)

    def _name(self, name):
        base, i = name, 1
        while name in self._bufs:
            i += 1
            name = "%s#%d" % (base, i)
        return name

    def check(self):
        """Every guard byte of every buffer is intact (synchronise first for device buffers)."""
        for name, (buf, lo, nbytes) in self._bufs.items():
            h = self._host(buf)
            for part, rel0 in ((h[:lo], -lo), (h[lo + nbytes:], nbytes)):
                bad = np.nonzero(part != self.canary)[0]
                if bad.size:
                    off = rel0 + int(bad[0])
                    raise AssertionError("%s: guard damaged at offset %d of the %d-byte view (0x%02x, canary 0x%02x; %d bytes damaged)" %
                                         (name, off, nbytes, part[bad[0]], self.canary, bad.size))

    def poisoned(self, view) -> bool:
        """Every byte of `view` still holds the canary (what an output must look like before its kernel runs)."""
        return bool((self._host(view).reshape(-1) == self.canary).all())


class DeviceArena(_Base):
    """Guarded device buffers (torch uint8 on cuda:`device`)."""

    def __init__(self, canary: int = CANARIES[0], device: int = 0):
        super().__init__(canary)
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)

    def _host(self, t):
        return t.cpu().numpy()

    def _alloc(self, name, nbytes, offset):
        buf = self.torch.full((GUARD + offset + nbytes + GUARD,), self.canary, dtype=self.torch.uint8, device=self.dev)
        lo = GUARD + offset
        self._bufs[self._name(name)] = (buf, lo, nbytes)
        return buf, lo

    def out(self, name, nbytes, shape=None):
        buf, lo = self._alloc(name, nbytes, VIEW_OFFSET)
        v = buf[lo:lo + nbytes]
        assert not nbytes or (v.data_ptr() % 16 == 0 and v.data_ptr() % 128 != 0), hex(v.data_ptr())
        return v.view(shape) if shape is not None else v

    def input(self, name, array):
        a = np.ascontiguousarray(array, np.uint8)
        buf, lo = self._alloc(name, a.nbytes, INPUT_OFFSET)
        v = buf[lo:lo + a.nbytes]
        v.copy_(self.torch.from_numpy(a.reshape(-1)).to(self.dev))
        assert v.data_ptr() % 4 == 0 and v.data_ptr() % 16 != 0, hex(v.data_ptr())
        return v.view(a.shape)

    def check(self):
        self.torch.cuda.synchronize(self.dev)
        super().check()

    def check_on_device(self):
        """check() for buffers too large to copy to the host: the same guard bytes, compared by torch on the device."""
        self.torch.cuda.synchronize(self.dev)
        for name, (buf, lo, nbytes) in self._bufs.items():
            for part, rel0 in ((buf[:lo], -lo), (buf[lo + nbytes:], nbytes)):
                bad = self.torch.nonzero(part != self.canary)
                if bad.numel():
                    at = int(bad[0])
                    raise AssertionError("%s: guard damaged at offset %d of the %d-byte view (0x%02x, canary 0x%02x; %d bytes damaged)" %
                                         (name, rel0 + at, nbytes, int(part[at]), self.canary, bad.numel()))

    def poisoned_on_device(self, view) -> bool:
        """poisoned() without the copy to the host."""
        v = view.contiguous().view(self.torch.uint8).reshape(-1)
        if v.numel() % 4 == 0 and v.data_ptr() % 4 == 0:  # word by word: a quarter of the temporary
            word = int.from_bytes(bytes([self.canary]) * 4, "little", signed=True)
            return bool((v.view(self.torch.int32) == word).all())
        return bool((v == self.canary).all())

    def repoison(self):
        """Every byte of every buffer, views and guards, back to the canary: a large buffer is used a second time."""
        for buf, _lo, _nbytes in self._bufs.values():
            buf.fill_(self.canary)

    def witness(self, pkg, n, layout, want_ct=True, key_slab=True, n_keys=None):
        """A Witness as Context.alloc_witness shapes it, every member guarded and poisoned."""
        cols = [self.out("xyz"[c], n * pkg.column_stride(layout, c)) for c in range(3)]
        ct = self.out("ct", n * 16, (n, 16)) if want_ct else None
        key = self.key_witness(pkg, n if n_keys is None else n_keys, layout, want_rk=False) if key_slab else None
        return pkg.Witness(cols[0], cols[1], cols[2], ct, key)

    def key_witness(self, pkg, m, layout, want_rk=True):
        w = self.out("w", m * pkg.WORDS_ROWS)
        kx, ky, kz = [self.out(("kx", "ky", "kz")[c], m * pkg.key_column_stride(layout, c)) for c in range(3)]
        rk = self.out("rk", m * 176, (m, 176)) if want_rk else None
        return pkg.KeyWitness(w, kx, ky, kz, rk)


class HostArena(_Base):
    """Guarded host buffers: pageable numpy arrays, or page-locked ones from aesw_host_alloc (pinned=True; close() frees them)."""

    def __init__(self, canary: int = CANARIES[0], pinned: bool = False, pkg=None):
        super().__init__(canary)
        self.pinned, self.pkg = pinned, pkg
        self._pinned = []

    def _host(self, a):
        return np.asarray(a)

    def out(self, name, nbytes, shape=None):
        total = GUARD + VIEW_OFFSET + nbytes + GUARD + 128
        if self.pinned:
            raw = self.pkg.api.host_alloc(total)
            self._pinned.append(raw)
        else:
            raw = np.empty(total, np.uint8)
        # place the view at VIEW_OFFSET past a 128-byte boundary whatever the base is
        start = GUARD + VIEW_OFFSET + (-(raw.ctypes.data + GUARD) % 128)
        buf = raw[start - GUARD - VIEW_OFFSET: start + nbytes + GUARD]
        buf[:] = self.canary
        lo = GUARD + VIEW_OFFSET
        self._bufs[self._name(name)] = (buf, lo, nbytes)
        v = buf[lo:lo + nbytes]
        assert not nbytes or (v.ctypes.data % 16 == 0 and v.ctypes.data % 128 != 0)
        return v.reshape(shape) if shape is not None else v

    def close(self):
        for a in self._pinned:
            self.pkg.api.host_free(a)
        self._pinned = []


# ---- C ABI calls whose Python wrappers allocate their own outputs ------------------------------------------------------

def _ptr(t):
    if t is None:
        return None
    return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data


def _slab(pkg, kw):
    return pkg.api.KeySlab(*[_ptr(t) for t in kw[:4]]) if kw is not None else None


def schedule_key(ctx, pkg, key, layout, slab):
    """aesw_schedule_key_device writing the key slab into `slab` (a guarded KeyWitness, or None for no slab)."""
    ks = _slab(pkg, slab)
    ctx._check(ctx._lib.aesw_schedule_key_device(ctx._h, key.data_ptr(), layout, C.byref(ks) if ks is not None else None,
                                                 ctx._stream()), "aesw_schedule_key_device")


def key_schedule(ctx, keys, layout, out):
    """aesw_key_schedule_witness_device for keys [n,16] into `out` (guarded KeyWitness; out.rk None: no round keys)."""
    n = keys.shape[0]
    ctx._check(ctx._lib.aesw_key_schedule_witness_device(ctx._h, keys.data_ptr(), n, layout, *[_ptr(t) for t in out],
                                                         ctx._stream()), "aesw_key_schedule_witness_device")


def lookup_table(ctx, cols):
    ctx._check(ctx._lib.aesw_lookup_table_device(ctx._h, *[_ptr(t) for t in cols], ctx._stream()), "aesw_lookup_table_device")


def encrypt_witness_host(ctx, pkg, pt, keys, n, layout, wit):
    """aesw_encrypt_witness (host pointers) into the guarded host Witness `wit`; keys None / [16] / [n,16]."""
    pbk = 0 if keys is None or keys.size == 16 else 1
    ks = _slab(pkg, wit.key)
    ctx._check(ctx._lib.aesw_encrypt_witness(ctx._h, _ptr(pt), _ptr(keys), pbk, n, layout,
                                             *[_ptr(c) if c.size else None for c in wit[:3]], _ptr(wit.ct),
                                             C.byref(ks) if ks is not None else None), "aesw_encrypt_witness")


def host_witness(arena, pkg, n, layout, n_keys):
    cols = [arena.out("xyz"[c], n * pkg.column_stride(layout, c)) for c in range(3)]
    key = pkg.KeyWitness(arena.out("w", n_keys * ol.WORDS_ROWS),
                         *[arena.out(("kx", "ky", "kz")[c], n_keys * pkg.key_column_stride(layout, c)) for c in range(3)], None)
    return pkg.Witness(cols[0], cols[1], cols[2], arena.out("ct", n * 16, (n, 16)), key)


def random_tables(seed=5):
    """Tables that are not xtime tables (the generic LDS-lookup path), as test_gpu_parity's test_generic_table_path builds them."""
    rng = np.random.default_rng(seed)
    return (rng.permutation(256).astype(np.uint8), rng.integers(0, 256, 256, dtype=np.uint8),
            rng.integers(0, 256, 256, dtype=np.uint8))
