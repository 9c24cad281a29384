"""What the GPU tests of libaesw_vanish.so share (a helper module, not a conftest): seeded column groups on the device, the
permutation's values gathered set by set, the accumulator driven segment by segment over guarded buffers, and the expected
quotient from tests/quot_model.py, computed once per case."""
import functools

import numpy as np

import ntt_model as nm
import quot_model as qm
import sigma_model as sm
import vanish_cases as vc

SEED = 0x766e7368


@functools.lru_cache(maxsize=None)
def columns(ext_k, n_sets, chunk_len):
    """(cells, values) of quot_model.seeded_columns"""
    return qm.seeded_columns(ext_k, n_sets, chunk_len, SEED + 64 * ext_k + 8 * n_sets + chunk_len)


def challenges(seed=0x7663686c):
    """theta, beta, gamma, y"""
    return tuple(nm.seeded_values(4, seed))


@functools.lru_cache(maxsize=None)
def expected(case, seed=0x7663686c, rows=None):
    """quot_model.quotient over the case's seeded columns, as cells: every row, or the rows of the tuple `rows`"""
    k, ext_k, zeta_sel, n_sets, chunk_len = case
    _cells, values = columns(ext_k, n_sets, chunk_len)
    return nm.to_cells(qm.quotient(k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), values, *challenges(seed), rows=rows))


def values_of_set(cells, n_sets, chunk_len, s):
    """uint8 [columns of set s, E, 32]: the permutation's value columns of that set, in the permutation's order"""
    first, end = sm.sets_of(sm.columns(n_sets), chunk_len)[s]
    sources = sm.sources(n_sets)
    return np.stack([cells["advice"][sources[c]] if sources[c] <= 3 * n_sets else cells["rcon"][0] for c in range(first, end)])


def upload(cells):
    """group -> a device tensor"""
    import torch
    return {g: torch.from_numpy(np.ascontiguousarray(c)).cuda() for g, c in cells.items()}


def put(arena, name, cells):
    """a guarded, 16-byte aligned device copy of uint8 cells"""
    import torch
    t = arena.out(name, cells.size, cells.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(cells)).to(t.device))
    return t


def fold(ctx, acc, d, values, n_sets):
    """every segment of the accumulator `acc` in its order over the device groups `d`; values[s]: the gathered columns of set s"""
    acc.head(d["advice"][3 * n_sets], d["rcon"], d["zperm"], d["l"])
    for s in range(acc.perm_sets):
        first = s * acc.chunk_len
        acc.permutation_set(s, values[s], d["sigma"][first:first + values[s].shape[0]], d["zperm"][s], d["l"])
    for s in range(n_sets):
        five = slice(5 * s, 5 * s + 5)
        acc.lookup_set(s, d["advice"][3 * s:3 * s + 3], d["selectors"][five], d["table"], d["a"][five], d["s"][five], d["zlookup"][five], d["l"])
    return acc.divide()
