"""The blinding cells of libaesw_blind.so on the GPU: Context.blind_rows and Context.blinding_tail against tests/blind_model.py
(hashlib.blake2b), cell for cell, on poisoned and guard-banded outputs.  k = 10 (and 11 once, so that the column stride is not the
only one tried), 1 and 3 columns, tails of 1, 6, 64, 65, 257 and 2^k rows -- 65 and 257 pass a wave and a 256-thread workgroup, and
n_cols * tail is a multiple of neither -- a first_column that is not 0, a domain above 2^32, the three "fr_store_mode"s.  Every byte
below first_row and in the guard bands keeps its poison; the compact tail equals the rows in place; two domains and two columns
under one seed differ."""
import numpy as np
import pytest

import blind_cases as bc
import blind_model as bm
import guarded as G

pytestmark = pytest.mark.gpu


def fill(pkg, ctx, arena, k, n_cols, tail, seed, domain, first_column):
    """(cells, compact): blind_rows into a poisoned [n_cols, 2^k, 32] and blinding_tail into a poisoned [n_cols, tail, 32]"""
    first_row = (1 << k) - tail
    assert int(pkg.api.load_blind_library().aesw_blind_tail_rows(k, first_row)) == tail
    cells = arena.out("cells", n_cols * 32 << k, (n_cols, 1 << k, 32))
    compact = arena.out("tail", n_cols * tail * 32, (n_cols, tail, 32))
    d_seed = ctx.blinding_seed(seed)
    assert ctx.blind_rows(cells, k, first_row, d_seed, domain, first_column) is cells
    assert ctx.blinding_tail(k, n_cols, first_row, d_seed, domain, first_column, out=compact) is compact
    arena.check()
    return cells.cpu().numpy(), compact.cpu().numpy()


def check(arena, k, n_cols, tail, seed, domain, first_column, cells, compact, what):
    first_row = (1 << k) - tail
    want = bm.tail_cells(seed, k, n_cols, first_row, domain, first_column)
    G.assert_bytes(what + ": the rows from first_row on", cells[:, first_row:], want)
    G.assert_bytes(what + ": the compact tail", compact, want)
    assert (cells[:, :first_row] == arena.canary).all(), what + ": a byte below first_row was written"


@pytest.mark.parametrize("n_cols", bc.COLS)
@pytest.mark.parametrize("tail", bc.FILL_TAILS)
def test_rows_and_tail_are_the_models_cells_and_nothing_else_is_written(pkg, ctx, n_cols, tail):
    canary = G.CANARIES[(n_cols + tail) % 2]
    arena = G.DeviceArena(canary)
    cells, compact = fill(pkg, ctx, arena, bc.K, n_cols, tail, bc.SEED, bc.BIG_DOMAIN, bc.FIRST_COLUMN)
    check(arena, bc.K, n_cols, tail, bc.SEED, bc.BIG_DOMAIN, bc.FIRST_COLUMN, cells, compact, "%d columns, %d rows" % (n_cols, tail))


@pytest.mark.parametrize("mode", bc.STORE_MODES)
def test_every_store_mode_writes_the_same_cells(pkg, ctx, mode):
    before = ctx.get_option("fr_store_mode")
    ctx.set_option("fr_store_mode", mode)
    try:
        arena = G.DeviceArena(G.CANARIES[mode % 2])
        cells, compact = fill(pkg, ctx, arena, bc.K, 3, 65, bc.SEEDS["ones"], bc.DOMAIN, 0)
    finally:
        ctx.set_option("fr_store_mode", before)
    check(arena, bc.K, 3, 65, bc.SEEDS["ones"], bc.DOMAIN, 0, cells, compact, "fr_store_mode %d" % mode)


def test_another_k_another_stride_and_the_seed_of_zeros(pkg, ctx):
    arena = G.DeviceArena(G.CANARIES[1])
    cells, compact = fill(pkg, ctx, arena, 11, 3, 6, bc.SEEDS["zeros"], bc.DOMAIN, (1 << 32) + 1)
    check(arena, 11, 3, 6, bc.SEEDS["zeros"], bc.DOMAIN, (1 << 32) + 1, cells, compact, "k = 11")


def test_domains_columns_and_seeds_part_the_cells(pkg, ctx):
    k, tail = bc.K, 6
    first_row = (1 << k) - tail
    seed = ctx.blinding_seed(bc.SEED)
    a = ctx.blinding_tail(k, 2, first_row, seed, 1).cpu().numpy()
    b = ctx.blinding_tail(k, 2, first_row, seed, 2).cpu().numpy()
    c = ctx.blinding_tail(k, 2, first_row, seed, 1, first_column=1).cpu().numpy()
    other = ctx.blinding_tail(k, 2, first_row, ctx.blinding_seed(bc.SEEDS["ones"]), 1).cpu().numpy()
    rows = lambda t: {r.tobytes() for r in t.reshape(-1, 32)}  # noqa: E731
    assert len(rows(a)) == 2 * tail and not rows(a) & rows(b) and not rows(a) & rows(other)  # two domains, two seeds: no cell shared
    assert not rows(a[0]) & rows(a[1]) and np.array_equal(a[1], c[0]) and not np.array_equal(a[0], c[0])  # column j + 1 is first_column + 1's column j
    fresh = ctx.blinding_seed()
    assert tuple(fresh.shape) == (32,) and fresh.is_cuda and not np.array_equal(fresh.cpu().numpy(), ctx.blinding_seed().cpu().numpy())  # the OS's randomness
    assert all(v < bm.R for v in (int.from_bytes(r, "little") for r in rows(a)))  # canonical
