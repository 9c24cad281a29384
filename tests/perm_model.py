"""plookup's permuted columns restated in numpy, from a histogram alone: repeat and cumsum, no search, no scan by hand and no line
shared with csrc/aesw_perm.h.  arrange() is the construction, relations() checks plookup's four relations on any (a, s) without
knowing how they were made.  Held against the header in tests/test_perm_model.py; the yardstick of tests/test_gpu_perm.py."""
import numpy as np

BINS = 66561
ZERO_ROW = 66560
SECTION = {1: (0, 256), 2: (512, 65536), 3: (256, 256), 4: (66048, 256), 5: (66304, 256)}  # tag -> (first table row, rows)
TAGS = (1, 2, 3, 4, 5)


def counts(hist, tag, u):
    """(c int64[BINS], overflowed): how often every table row is an input of the argument over u rows."""
    first, n = SECTION[tag]
    h = np.asarray(hist).astype(np.int64)[first:first + n] & 0xFFFFFFFF  # a bin is an unsigned word, however the tensor types it
    before = np.cumsum(h) - h
    c = np.zeros(BINS, np.int64)
    c[first:first + n] = np.clip(u - before, 0, h)
    c[ZERO_ROW] = u - c.sum()
    assert c[ZERO_ROW] >= 0 and c.sum() == u
    return c, bool(h.sum() > u)


def arrange(hist, tag, u, pad_row):
    """(a int64[u], s int64[u], overflowed) of one argument."""
    assert BINS <= u and 0 <= pad_row < BINS
    c, over = counts(hist, tag, u)
    rows = np.arange(BINS)
    a = np.repeat(rows, c)
    used = c > 0
    starts = (np.cumsum(c) - c)[used]
    s = np.full(u, -1, np.int64)
    s[starts] = rows[used]
    left = np.concatenate([rows[~used], np.full(u - BINS, pad_row, np.int64)])
    assert left.size == u - starts.size
    s[s < 0] = left
    return a, s, over


def table_column(u, pad_row):
    """The table column over u rows as row indices: the 66 561 rows, then pad_row."""
    return np.concatenate([np.arange(BINS), np.full(u - BINS, pad_row, np.int64)])


def relations(a, s, inputs_count, u, pad_row):
    """None, or which of plookup's relations (a, s) misses.  inputs_count int64[BINS]: how often every row is an input."""
    a, s = np.asarray(a).astype(np.int64), np.asarray(s).astype(np.int64)
    if a.shape != (u,) or s.shape != (u,) or a.min() < 0 or s.min() < 0 or a.max() >= BINS or s.max() >= BINS:
        return "shape or range"
    if not np.array_equal(np.bincount(a, minlength=BINS), inputs_count):
        return "A' is no permutation of the inputs"
    if not np.array_equal(np.bincount(s, minlength=BINS), np.bincount(table_column(u, pad_row), minlength=BINS)):
        return "S' is no permutation of the table column"
    if a[0] != s[0]:
        return "A'[0] != S'[0]"
    bad = np.nonzero((a[1:] != s[1:]) & (a[1:] != a[:-1]))[0]
    if bad.size:
        return "A'[%d] is neither S'[%d] nor A'[%d]" % (bad[0] + 1, bad[0] + 1, bad[0])
    return None


def report(hists, u):
    """What aesw_perm_report holds after a build over int [n_sets, BINS] histograms: the dict of api.perm_report_dict."""
    over = [(s, t) for s in range(len(hists)) for t in TAGS if counts(hists[s], t, u)[1]]
    return {"arguments": 5 * len(hists), "overflowed": len(over), "first_overflow": min(over) if over else None}


# ---- the histogram kinds of the tests: every bin OUTSIDE the argument's section holds `garbage` ------------------------------

def synthetic(kind, tag, u, rng, garbage=0xFFFFFFFF):
    """uint32[BINS]; kinds: empty, one_bin, all_ones, exact (the section sums to u), over1 / over_big (to u + 1 / u + 2^20),
    random."""
    first, n = SECTION[tag]
    h = np.full(BINS, garbage, np.uint64)
    sec = np.zeros(n, np.uint64)
    if kind == "one_bin":
        sec[int(rng.integers(0, n))] = u - 7
    elif kind == "all_ones":
        sec[:] = 1
    elif kind in ("exact", "over1", "over_big", "random"):
        total = {"exact": u, "over1": u + 1, "over_big": u + (1 << 20), "random": u // 3}[kind]
        cut = np.sort(rng.integers(0, total + 1, n - 1))
        sec[:] = np.diff(np.concatenate([[0], cut, [total]]))
        sec[rng.integers(0, n, n // 3)] = 0  # holes; the sum is restored in one bin
        sec[int(rng.integers(0, n))] += total - int(sec.sum())
        assert int(sec.sum()) == total
    else:
        assert kind == "empty", kind
    h[first:first + n] = sec
    return h.astype(np.uint32)
