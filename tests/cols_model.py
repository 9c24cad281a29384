"""The test model of aesw_cols_check_device (include/aesw_cols.h), on the host: the assembled advice columns of one circuit are
DE-ASSEMBLED into DENSE slabs with aesw_block_placement and numpy and handed to the CPU run of aesw_check.h (tests/lane_model,
the model tests/test_check_model.py holds against the oracle's verifier and tests/test_gpu_circ_check.py composes its expected
reports from); stray cells (never assigned, not 0) and non-canonical Fr cells are counted with numpy.  Nothing here runs the
kernel or reads its source: the never-assigned cells come from the packed-index tables, the Fr table from the modulus.

A circuit's result is a tuple R = (lookup, copy, gate, input, first, cell_failures, unassigned_failures, first_cell) with
`first` and `first_cell` in the batch's numbering (NONE when there is none); compose() adds circuits up to the report dict
Context.check_columns returns."""
import ctypes as C

import numpy as np

NONE = 2 ** 64 - 1
AES_ROWS, KEY_ROWS, WORDS_ROWS = 1360, 400, 96
FR_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # bn256::Fr
COUNTS = ("lookup_failures", "copy_failures", "gate_failures", "input_failures")


def fr_table():
    """Fp::from(u64) of a byte: v * 2^256 mod r, 32 bytes little-endian."""
    return np.stack([np.frombuffer(((v << 256) % FR_MOD).to_bytes(32, "little"), np.uint8) for v in range(256)])


def load_lane_model():
    import __graft_entry__ as ge
    L = C.CDLL(str(ge.build_lane_model()))
    L.lane_model_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 9
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ColsModel:
    def __init__(self, lane_model, tab768, pkg, k, n_sets, offsets):
        self.L, self.tab, self.pkg, self.k, self.n_sets = lane_model, np.ascontiguousarray(tab768, np.uint8), pkg, k, n_sets
        self.offs = [int(v) for v in offsets]
        self.nc, self.n = len(self.offs) - 1, self.offs[-1]
        self.ncol, self.rows = 3 * n_sets + 1, 1 << k
        cap = pkg.block_capacity(k, n_sets)
        assert self.offs[0] == 0 and all(0 <= b - a <= cap for a, b in zip(self.offs, self.offs[1:])), "the model takes valid offsets"
        self.enc_assigned = [pkg.packed_index(c) >= 0 for c in range(3)]
        self.key_assigned = [pkg.key_packed_index(c) >= 0 for c in range(3)]
        self.place = [pkg.block_placement(k, n_sets, j) for j in range(max(b - a for a, b in zip(self.offs, self.offs[1:])))]
        self.lut = fr_table()
        lo = self.lut[:, :8].copy().view(np.uint64).reshape(256)
        assert len(set(lo.tolist())) == 256
        self.lut_order = np.argsort(lo)
        self.lut_lo = lo[self.lut_order]

    def cells(self):
        return self.nc * self.ncol * self.rows

    def cell_index(self, c, col, row):
        return ((c * self.ncol + col) << self.k) + row

    def assigned(self, c):
        """bool [ncol, rows]: the cells of circuit c some DENSE-slab assigned cell maps to."""
        a = np.zeros((self.ncol, self.rows), bool)
        for col in range(3):
            a[col, :KEY_ROWS] = self.key_assigned[col]
        a[self.ncol - 1, :WORDS_ROWS] = True
        for j in range(self.offs[c + 1] - self.offs[c]):
            s, r = self.place[j]
            for col in range(3):
                a[3 * s + col, r:r + AES_ROWS] = self.enc_assigned[col]
        return a

    def to_bytes(self, cols):
        """[ncol, rows] bytes and the bool [ncol, rows] of canonical cells from one circuit's columns in either form; a
        non-canonical cell gives byte 0 (the header leaves it unspecified)."""
        cols = np.ascontiguousarray(cols)
        if cols.ndim == 2:
            assert cols.shape == (self.ncol, self.rows)
            return cols, np.ones(cols.shape, bool), cols != 0
        assert cols.shape == (self.ncol, self.rows, 32)
        flat = cols.reshape(-1, 32)
        lo = flat[:, :8].copy().view(np.uint64).reshape(-1)
        pos = np.clip(np.searchsorted(self.lut_lo, lo), 0, 255)
        cand = self.lut_order[pos]
        canon = (self.lut[cand] == flat).all(axis=1)
        b = np.where(canon, cand, 0).astype(np.uint8)
        return b.reshape(self.ncol, self.rows), canon.reshape(self.ncol, self.rows), flat.any(axis=1).reshape(self.ncol, self.rows)

    def slabs(self, c, b):
        """DENSE slabs of circuit c out of its byte matrix b: x, y, z [n_c * 1360], w [96], kx, ky, kz [400]."""
        n_c = self.offs[c + 1] - self.offs[c]
        xyz = [np.zeros((n_c, AES_ROWS), np.uint8) for _ in range(3)]
        for j in range(n_c):
            s, r = self.place[j]
            for col in range(3):
                xyz[col][j] = b[3 * s + col, r:r + AES_ROWS]
        key = [np.ascontiguousarray(b[col, :KEY_ROWS]) for col in range(3)]
        return [np.ascontiguousarray(a.reshape(-1)) for a in xyz], np.ascontiguousarray(b[self.ncol - 1, :WORDS_ROWS]), key

    def _lane(self, pt, key, n, xyz, ct, w, kxyz):
        rep = np.zeros(7, np.uint64)
        dummy = np.zeros(16, np.uint8)
        x, y, z = xyz if n else (dummy, dummy, dummy)
        assert self.L.lane_model_check(_p(self.tab), 0, _p(pt if n else dummy), _p(key), 0, n, _p(x), _p(y), _p(z), _p(ct) if n else None,
                                       _p(w), _p(kxyz[0]), _p(kxyz[1]), _p(kxyz[2]), _p(rep)) == 0
        return [int(v) for v in rep]

    def circuit(self, c, cols, pt, keys, ct):
        """R of circuit c.  cols: its [ncol, rows] bytes or [ncol, rows, 32] Fr cells; pt [n,16], keys [C,16] or None, ct [n,16] or
        None are the batch's."""
        lo, hi = self.offs[c], self.offs[c + 1]
        b, canon, nonzero = self.to_bytes(cols)
        stray = ~self.assigned(c) & nonzero
        bad = np.flatnonzero((stray | ~canon).reshape(-1))
        first_cell = NONE if bad.size == 0 else self.cell_index(c, 0, 0) + int(bad[0])
        xyz, w, kxyz = self.slabs(c, b)
        key = None if keys is None else np.ascontiguousarray(keys[c])
        pt_c = np.ascontiguousarray(pt[lo:hi])
        ct_c = None if ct is None else np.ascontiguousarray(ct[lo:hi])
        kr = self._lane(None, key, 0, None, None, w, kxyz)
        kfirst = NONE if kr[6] == NONE else (c << 20) | (kr[6] & 0xFFFFF)
        tot = self._lane(pt_c, key, hi - lo, xyz, ct_c, w, kxyz)
        bfirst = NONE
        if tot[2:6] != kr[2:6]:  # some block fails: the smallest such check, in the batch's numbering
            for j in range(hi - lo):
                one = self._lane(pt_c[j:j + 1], key, 1, [a[j * AES_ROWS:(j + 1) * AES_ROWS] for a in xyz],
                                 None if ct_c is None else ct_c[j:j + 1], w, kxyz)
                if one[2:6] != kr[2:6]:
                    f = one[6]
                    assert not (f >> 19) & 1  # unit 0 both, and a block's checks sort before its key slab's
                    bfirst = ((lo + j) << 20) | (f & 0xFFFFF)
                    break
            assert bfirst != NONE
        return (tot[2], tot[3], tot[4], tot[5], min(kfirst, bfirst), int((~canon).sum()), int(stray.sum()), first_cell)

    def compose(self, per_circuit, offset_failures=0):
        tot = [sum(r[i] for r in per_circuit) for i in range(4)]
        f = min(r[4] for r in per_circuit)
        fc = min(r[7] for r in per_circuit)
        cell, unas = sum(r[5] for r in per_circuit), sum(r[6] for r in per_circuit)
        out = {"blocks": self.n, "keys": self.nc, "first": None if f == NONE else (f >> 20, bool((f >> 19) & 1), (f >> 16) & 7, f & 0xFFFF),
               "offset_failures": offset_failures, "cell_failures": cell, "unassigned_failures": unas,
               "first_cell": None if fc == NONE else fc, "cells": self.cells(),
               "satisfied": not any(tot) and not cell and not unas and not offset_failures}
        out.update(dict(zip(COUNTS, tot)))
        return out

    def check(self, cols, pt, keys, ct):
        """The whole batch: cols [C, ncol, rows(, 32)]."""
        return self.compose([self.circuit(c, cols[c], pt, keys, ct) for c in range(self.nc)])
