"""The lookup multiplicities restated in numpy, from what the PROVER holds: the assembled advice columns as bytes and the
selector columns.  Nothing here knows a slab, a layout, a packed index or where a circuit places a block: a row counts because
its selector is on, and its operands are the cells of its own row.  Held against the oracle's circuit in
tests/test_mult_model.py, and the yardstick of tests/test_gpu_mult.py."""
import numpy as np

BINS = 66561
# selector i of a set (aesw_assemble_selectors: range, xor, sbox, mul2, mul3) -> (first table row, rows) of its section
SECTIONS = ((0, 256), (512, 65536), (256, 256), (66048, 256), (66304, 256))
TAGS = (1, 2, 3, 4, 5)  # the tag column of the table for selector i


def section_sums(hist):
    """[..., 5]: the sum of every section of histogram(s) [..., 66561], in selector order."""
    hist = np.asarray(hist)
    return np.stack([hist[..., f:f + n].sum(axis=-1) for f, n in SECTIONS], axis=-1)


def multiplicities(advice, selectors, tables):
    """advice uint8[3 * n_sets + 1, rows], selectors uint8[5 * n_sets + 1, rows], tables (sbox, mul2, mul3) -> (hist
    int64[n_sets, 66561], misses): per set and selector, every enabled row looks up (x, y, z) of its own row; the bin is the
    table row with those INPUTS, and the row is a miss where the table's output there is not the row's."""
    advice, selectors = np.asarray(advice), np.asarray(selectors)
    n_sets = (advice.shape[0] - 1) // 3
    assert advice.shape[0] == 3 * n_sets + 1 and selectors.shape[0] == 5 * n_sets + 1 and advice.shape[1] == selectors.shape[1]
    sbox, mul2, mul3 = [np.asarray(t, np.int64) for t in tables]
    hist, misses = np.zeros((n_sets, BINS), np.int64), 0
    for s in range(n_sets):
        for i, (first, _n) in enumerate(SECTIONS):
            on = np.nonzero(selectors[5 * s + i])[0]
            x, y, z = [advice[3 * s + c][on].astype(np.int64) for c in range(3)]
            if i == 0:
                bins, hit = first + x, np.ones(on.size, bool)
            elif i == 1:
                bins, hit = first + 256 * x + y, z == (x ^ y)
            else:
                bins, hit = first + x, y == (sbox, mul2, mul3)[i - 2][x]
            hist[s] += np.bincount(bins[hit], minlength=BINS)
            misses += int((~hit).sum())
    return hist, misses


BLOCK_ROWS, KEY_ROWS = 1360, 400


def _rows(advice, selectors, tables, s, first, n):
    """(hist int64[66561], misses) of rows [first, first + n) of set s alone: multiplicities over the slice of the set's three
    advice and five selector columns, as a circuit of one set (its last advice and last selector column play no part)."""
    advice, selectors = np.asarray(advice), np.asarray(selectors)
    pad = np.zeros((1, n), np.uint8)
    a3, s5 = advice[3 * s:3 * s + 3, first:first + n], selectors[5 * s:5 * s + 5, first:first + n]
    assert a3.shape == (3, n) and s5.shape == (5, n), "rows %d ... %d of set %d are not all there" % (first, first + n, s)
    hist, misses = multiplicities(np.concatenate([a3, pad]), np.concatenate([s5, pad]), tables)
    return hist[0], misses


def block_histograms(advice, selectors, tables, places):
    """(hist int64[len(places), 66561], misses int64[len(places)]): for every (set, first row) of `places` -- where the circuit
    placed a block -- what the block's 1 360 rows look up.  Which blocks a circuit counts, and into which set, is the caller's
    to say: nothing here knows a slab index or an offset list."""
    hist, misses = np.zeros((len(places), BINS), np.int64), np.zeros(len(places), np.int64)
    for i, (s, first) in enumerate(places):
        hist[i], misses[i] = _rows(advice, selectors, tables, s, first, BLOCK_ROWS)
    return hist, misses


def key_histogram(advice, selectors, tables):
    """(hist int64[66561], misses) of the key schedule's rows: rows 0 ... 399 of set 0."""
    return _rows(advice, selectors, tables, 0, 0, KEY_ROWS)
