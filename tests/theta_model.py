"""The two rules of libaesw_theta.so restated in numpy and Python ints, from what the PROVER holds and with no line shared with
csrc/aesw_theta.h or csrc/aesw_fr.h: (1) the three compressed tables from the four byte columns of the lookup table --
acc = acc * theta + e over the first 2, 3 or 4 columns, in plain integers mod r, put into Montgomery bytes at the end --;
(2) the input index column of every argument from a circuit's advice matrix and selector columns: where the argument's selector
is on, the table row with the row's inputs, or the miss marker where that row's output is not the row's; the all-zero row
everywhere else.  Held against the header in tests/test_theta_model.py; the yardstick of the tests/test_gpu_theta_*.py."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
BINS = 66561
ZERO_ROW = 66560
MISS = 0xFFFFFFFF
TAGS = (1, 2, 3, 4, 5)
TABLE_OF_TAG = {1: 0, 2: 2, 3: 1, 4: 1, 5: 1}  # arity 2: the range check; 3: S-box and the two products; 4: xor
# selector i of a set (aesw_assemble_selectors: range, xor, sbox, mul2, mul3) -> (first table row, rows) of its section
SECTIONS = ((0, 256), (512, 65536), (256, 256), (66048, 256), (66304, 256))


def cell(value):
    """bytes: the 32-byte cell of an integer mod r"""
    return ((value % R) * (1 << 256) % R).to_bytes(32, "little")


def cells(values):
    return np.frombuffer(b"".join(cell(v) for v in values), np.uint8).reshape(-1, 32)


def value(cell_bytes):
    """the integer a canonical cell stands for"""
    return int.from_bytes(bytes(cell_bytes), "little") * pow(1 << 256, -1, R) % R


def compressed_values(table, theta):
    """[3][66561] Python ints: table uint8[4, 66561] (tag, a, b, c) compressed over its first j + 2 columns."""
    cols = [[int(v) for v in table[i]] for i in range(4)]
    out = []
    for arity in (2, 3, 4):
        acc = cols[0]
        for i in range(1, arity):
            acc = [(a * theta + e) % R for a, e in zip(acc, cols[i])]
        out.append(acc)
    return out


def compressed_tables(table, theta):
    """uint8[3, 66561, 32]; all zero for a theta that is not canonical."""
    if not 0 <= theta < R:
        return np.zeros((3, BINS, 32), np.uint8)
    return np.stack([cells(t) for t in compressed_values(table, theta)])


def input_columns(advice, selectors, tables):
    """(index int64[n_sets, 5, rows], lookups, misses): advice uint8[3 * n_sets + 1, rows], selectors uint8[5 * n_sets + 1, rows],
    tables (sbox, mul2, mul3)."""
    advice, selectors = np.asarray(advice), np.asarray(selectors)
    n_sets, rows = (advice.shape[0] - 1) // 3, advice.shape[1]
    assert advice.shape[0] == 3 * n_sets + 1 and selectors.shape == (5 * n_sets + 1, rows)
    sbox, mul2, mul3 = [np.asarray(t, np.int64) for t in tables]
    out = np.full((n_sets, 5, rows), ZERO_ROW, np.int64)
    lookups = misses = 0
    for s in range(n_sets):
        x, y, z = [advice[3 * s + c].astype(np.int64) for c in range(3)]
        for i, (first, _n) in enumerate(SECTIONS):
            on = selectors[5 * s + i] != 0
            if i == 0:
                bins, hit = first + x, np.ones(rows, bool)
            elif i == 1:
                bins, hit = first + 256 * x + y, z == (x ^ y)
            else:
                bins, hit = first + x, y == (sbox, mul2, mul3)[i - 2][x]
            tag = TAGS[i]
            out[s, tag - 1][on] = np.where(hit, bins, MISS)[on]
            lookups += int(on.sum())
            misses += int((on & ~hit).sum())
    return out, lookups, misses


def table_column(u, pad_row):
    """The table column over u rows as row indices: the 66 561 rows, then pad_row."""
    return np.concatenate([np.arange(BINS), np.full(u - BINS, pad_row, np.int64)])


def gather(tables_fr, index, u):
    """uint8[n_sets, 5, u, 32]: what aesw_theta_columns_device writes below row u for index int [n_sets, 5, >= u]."""
    index = np.asarray(index).astype(np.int64) & 0xFFFFFFFF
    out = np.zeros(index.shape[:2] + (u, 32), np.uint8)
    for t in TAGS:
        idx = index[:, t - 1, :u]
        ok = idx < BINS
        out[:, t - 1] = np.where(ok[..., None], tables_fr[TABLE_OF_TAG[t]][np.minimum(idx, BINS - 1)], 0)
    return out
