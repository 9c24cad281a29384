"""The case lists of tests/test_gpu_vanish_*.py and the kernels they launch (imports without a GPU).  tests/test_vanish_library.py
holds every kernel of libaesw_vanish.so against launched()."""
import numpy as np

# (k, ext_k, zeta_sel, n_sets, chunk_len): every output cell is held at these
FULL = ((10, 12, 1, 1, 3),   # one column set; the last permutation set holds two columns of three
        (10, 12, 0, 2, 2),   # the other zeta, two column sets, four permutation sets
        (10, 13, 1, 2, 3))   # m = 8
SPLIT = (10, 15, 1, 1, 3)    # 2^15 rows: the index of x_j's low table carries at 2^14; held on split_rows()
BLIND = 6                    # n_rows = 2^k - BLIND
STORE_MODES = (0, 1, 2)      # "fr_store_mode": one instantiation of every segment kernel and of the division each
SEEDED_ROWS = 512
NAMESPACE = "aesw_vanish"


def n_rows(k):
    return (1 << k) - BLIND


def split_rows(k, ext_k, seed=0x73706c):
    """Every place a rotation wraps or the table index carries: rows 0 ... 2m and E - 2m ... E - 1 (next and prev wrap), the 2m rows
    on each side of 2^14 (the low table's index carries), the 2m rows on each side of E - n_rows * m (far wraps), and 512 seeded rows."""
    m, E = 1 << (ext_k - k), 1 << ext_k
    far = E - n_rows(k) * m
    rows = set(range(2 * m + 1)) | set(range(E - 2 * m, E)) | set(range((1 << 14) - 2 * m, (1 << 14) + 2 * m)) | set(range(far - 2 * m, far + 2 * m))
    rows |= {int(j) for j in np.random.default_rng(seed).integers(0, E, SEEDED_ROWS)}
    assert all(0 <= j < E for j in rows) and far == BLIND * m
    return sorted(rows)


def launched():
    return {"%s::vanish_%s_kernel" % (NAMESPACE, name) for name in ("tables", "scalars")} | \
        {"%s::vanish_%s_kernel<%d>" % (NAMESPACE, name, m) for name in ("head", "perm", "lookup", "divide") for m in STORE_MODES}
