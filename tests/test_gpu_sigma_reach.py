"""aesw_sigma_product_device on the GPU where the sweeps of tests/test_gpu_sigma_product.py never reach (tests/sigma_cases.py:
sc.MANY_SETS, sc.MANY_CHUNKS, sc.ZERO_EDGES), against tests/sigma_model.py in Python integers -- product_batched, which
tests/test_sigma_model.py holds equal to the literal product: every written cell of Z, every closing cell, the report, and the
poison (tests/guarded.py) above row min(n_rows, 2^k - 1) and in the guard bands, byte for byte.

  * More than 64 and more than 256 sets: sigma_chain_kernel joins its lanes by shuffles at every offset, its waves through LDS
    and its turns through `running`; a zero term in a late set is named by (set << k) + row.  The worlds close, and no two
    closing cells are equal: a carry that leaks between lanes, waves or turns shows.
  * 256 and 257 chunks: sigma_carry_kernel's scans end on the loop's bound, and take a second turn -- upwards with chunk 256
    in it, downwards with chunk 0 -- and its strided fold of the chunks' words meets a later zero term before an earlier one.
  * A zero term at every edge of a lane, a chunk and a set: lane_terms walks its rows downwards and counts, the chunk and the carry
    kernel fold a minimum, and the scan kernel keeps the rows up to the first zero term and no more.

The worlds and the planted zero terms are sc.world and sc.planted_zeros; the call and the comparison are those of
tests/test_gpu_sigma_product.py."""
import numpy as np
import pytest

import guarded as G
import sigma_cases as sc
import sigma_model as sm
import test_gpu_sigma_product as sp

pytestmark = pytest.mark.gpu
BETA, GAMMA = sp.BETA, sp.GAMMA
CLOSED = {"open": False, "zero_terms": 0, "first_zero": None, "out_of_range": 0, "noncanonical": False}
ids = lambda s: "k%d-c%d-l%d-u%d" % s  # noqa: E731

_worlds = {}


def world(shape, seed):
    if (shape, seed) not in _worlds:
        _worlds[shape, seed] = sc.world(shape[0], shape[1], shape[3], seed)
    return _worlds[shape, seed]


def closes(pkg, ctx, shape, seed, canary):
    """The world of `shape` closes on the device as in the model, cell for cell; the model, for what a case adds."""
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping = world(shape, seed)
    model = sm.product_batched(k, list(columns), mapping, BETA, GAMMA, chunk_len, n_rows)
    sets = -(-n_cols // chunk_len)
    assert model[1] == dict(CLOSED, sets=sets) and model[0][0][0] == 1 and model[0][-1][n_rows] == 1
    assert len({col[n_rows] for col in model[0]}) == sets  # the closing cells are pairwise distinct
    arena = G.DeviceArena(canary)
    got = sp.product(pkg, ctx, arena, shape, buffers, source, mapping, sp.cell(sp.mont(BETA)), sp.cell(sp.mont(GAMMA)))
    assert sp.held(pkg, arena, shape, got, model, shape) == dict(CLOSED, sets=sets)
    assert bytes(got[0][0, 0].cpu().numpy()) == sm.ONE_CELL and bytes(got[1][-1].cpu().numpy()) == sm.ONE_CELL
    return model


def zeroes_behind(pkg, ctx, shape, seed, cells, target, canary, what):
    """Zero denominators planted at `cells` (column, row): the model counts them, names the lowest (set, row) and is non-zero up
    to that row of that set and zero behind it, closing cells included -- stated before the device is looked at, which then
    agrees cell for cell."""
    k, n_cols, chunk_len, n_rows = shape
    buffers, source, columns, mapping, gamma = sc.planted_zeros(k, world(shape, seed), cells, target, BETA)
    model = sm.product_batched(k, list(columns), mapping, BETA, gamma, chunk_len, n_rows)
    at = sorted({(c // chunk_len, i) for c, i in cells})
    assert len(at) == len(cells)
    st, row = at[0]
    assert model[1] == {"sets": -(-n_cols // chunk_len), "open": True, "zero_terms": len(cells), "first_zero": (st << k) + row, "out_of_range": 0,
                        "noncanonical": False}, (what, model[1])
    z = model[0]
    assert all(all(col) for col in z[:st]) and all(z[st][:row + 1]) and not any(z[st][row + 1:]) and not any(any(col) for col in z[st + 1:]), what
    arena = G.DeviceArena(canary)
    got = sp.product(pkg, ctx, arena, shape, buffers, source, mapping, sp.cell(sp.mont(BETA)), sp.cell(sp.mont(gamma)))
    sp.held(pkg, arena, shape, got, model, what)
    return model


# ---- many sets -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sc.MANY_SETS, ids=ids)
def test_a_chain_of_more_sets_than_a_wave_and_than_a_turn_closes_cell_for_cell(pkg, ctx, shape):
    closes(pkg, ctx, shape, 0x7372 + sc.MANY_SETS.index(shape), G.CANARIES[sc.MANY_SETS.index(shape) % 2])


def test_the_delta_table_of_300_columns_is_the_models(pkg, ctx):
    k, n_cols = sc.MANY_SETS[0][:2]
    exp = sm.tables(k, n_cols)
    assert len(exp) == 1024 + 1 + 300 and exp[-1] == pow(sm.DELTA, 299, sm.R)
    arena = G.DeviceArena(G.CANARIES[1])
    out = arena.out("tables", 32 * len(exp), (len(exp), 32))
    got = ctx.permutation_tables(k, n_cols, _out=out)
    arena.check()
    bad = np.argwhere((got.cpu().numpy() != sm.cells(exp)).any(axis=1))
    assert not bad.size, "%d cells differ, first %d" % (len(bad), bad[0][0])


def test_zero_terms_in_the_second_wave_and_in_the_second_turn_name_the_first_and_zero_every_set_behind_it(pkg, ctx):
    shape = sc.MANY_SETS[0]
    assert shape[2] == 1 and [s for s, _ in sc.MANY_SETS_ZEROS] == [70, 260]  # a set is a column; lane 6 of wave 1, thread 4 of the second turn
    model = zeroes_behind(pkg, ctx, shape, 0x7372, sc.MANY_SETS_ZEROS, (0, 700), G.CANARIES[0], "sets 70 and 260")
    assert model[1]["zero_terms"] == 2 and model[1]["first_zero"] == (70 << 10) + sc.MANY_SETS_ZEROS[0][1]
    assert all(all(col) for col in model[0][:70]) and not any(any(col) for col in model[0][71:])


# ---- many chunks ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sc.MANY_CHUNKS, ids=ids)
def test_a_carry_over_256_and_over_257_chunks_closes_cell_for_cell(pkg, ctx, shape):
    k, _n_cols, _chunk_len, n_rows = shape
    assert min(n_rows, (1 << k) - 1) // 1024 + 1 == 256 + sc.MANY_CHUNKS.index(shape)
    closes(pkg, ctx, shape, 0x7363 + sc.MANY_CHUNKS.index(shape), G.CANARIES[sc.MANY_CHUNKS.index(shape) % 2])


def test_zero_terms_in_chunk_256_and_in_chunk_3_name_the_one_in_chunk_3(pkg, ctx):
    shape = sc.MANY_CHUNKS[1]
    assert [i // 1024 for _, i in sc.MANY_CHUNKS_ZEROS] == [256, 3] and all(c // shape[2] == 0 for c, _ in sc.MANY_CHUNKS_ZEROS)
    model = zeroes_behind(pkg, ctx, shape, 0x7364, sc.MANY_CHUNKS_ZEROS, (2, 70000), G.CANARIES[0], "chunks 256 and 3")
    assert model[1]["first_zero"] == sc.MANY_CHUNKS_ZEROS[1][1]


# ---- a zero term at every edge -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.ZERO_EDGES))
def test_a_zero_term_at_an_edge_of_a_lane_a_chunk_or_a_set_zeroes_what_lies_behind_it_and_no_more(pkg, ctx, name):
    shape, cells = sc.ZERO_SHAPE, sc.ZERO_EDGES[name]
    k, _n_cols, chunk_len, n_rows = shape
    model = zeroes_behind(pkg, ctx, shape, 0x737a, cells, sc.ZERO_TARGET, G.CANARIES[sorted(sc.ZERO_EDGES).index(name) % 2], name)
    z, first = model[0], model[1]["first_zero"]
    if name == "two_in_a_lane":
        assert [i % 4 for _, i in cells] == [1, 3] and cells[0][1] // 4 == cells[1][1] // 4 and first == (1 << k) + cells[0][1]
    elif name == "a_lanes_first_row":
        assert cells[0][1] % 4 == 0 and first == (1 << k) + cells[0][1]
    elif name == "a_chunks_last_and_next_first":
        assert [i for _, i in cells] == [2047, 2048] and len({c // chunk_len for c, _ in cells}) == 1 and first == (1 << k) + 2047
    elif name == "row_0_of_set_0":
        assert first == 0 and z[0][0] == 1 and not any(z[0][1:]) and not any(z[1]) and not any(z[2])
    elif name == "the_last_row_of_the_last_set":
        assert first == (2 << k) + n_rows - 1 and all(all(col[:n_rows]) for col in z) and [bool(col[n_rows]) for col in z] == [True, True, False]
    else:
        assert name == "two_sets" and [c // chunk_len for c, _ in cells] == [1, 2] and first == (1 << k) + cells[0][1]
