"""halo2's lookup grand product restated in Python integers, with no line shared with csrc/aesw_grand.h or csrc/aesw_fr.h: the
inverse is pow(x, r - 2, r) with 0 for 0 (the convention of ff's batch_invert), one per distinct value; the product is
  f[i] = (T[in[i]] + beta) * (T[tidx(i)] + gamma) * inv(T[a[i]] + beta) * inv(T[s[i]] + gamma),   Z[0] = 1, Z[i + 1] = Z[i] * f[i]
on plain residues, put into Montgomery bytes at the end.  An index at or above the table's 66 561 rows reads the all-zero row.
Held against the header in tests/test_grand_model.py; the yardstick of the tests/test_gpu_grand_*.py."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
M = 1 << 256
M_INV = pow(M, -1, R)
BINS = 66561
ZERO_ROW = 66560
TAGS = (1, 2, 3, 4, 5)
TABLE_OF_TAG = {1: 0, 2: 2, 3: 1, 4: 1, 5: 1}
ONE_CELL = (M % R).to_bytes(32, "little")

_inverse = {0: 0}  # residue -> its inverse: a pow per distinct value of the whole run


def inv(x):
    y = _inverse.get(x)
    if y is None:
        y = _inverse[x] = pow(x, R - 2, R)
    return y


def values(cells):
    """the residues uint8[..., 32] canonical cells stand for, as a flat list"""
    raw = np.ascontiguousarray(cells, np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") * M_INV % R for row in raw]


def cells(residues):
    """uint8[n, 32]: the Montgomery cells of residues"""
    return np.frombuffer(b"".join((v * M % R).to_bytes(32, "little") for v in residues), np.uint8).reshape(-1, 32)


def inverse_tables(tables_fr, beta, gamma):
    """(uint8[2, 3, 66561, 32], zero_terms) from the three compressed tables uint8[3, 66561, 32]: plane 0 inv(T + beta), plane 1
    inv(T + gamma); all zero, with no zero term counted, when beta or gamma is not canonical."""
    if not (0 <= beta < R and 0 <= gamma < R):
        return np.zeros((2, 3, BINS, 32), np.uint8), 0
    t = values(tables_fr)
    out, zeros = [], 0
    for c in (beta, gamma):
        sums = [(v + c) % R for v in t]
        zeros += sum(1 for v in sums if v == 0)
        out.append(cells([inv(v) for v in sums]).reshape(3, BINS, 32))
    return np.stack(out), zeros


def row_of_index(index):
    index = np.asarray(index).astype(np.int64) & 0xFFFFFFFF
    return np.where(index < BINS, index, ZERO_ROW)


def table_column(n, pad_row):
    i = np.arange(n)
    return np.where(i < BINS, i, pad_row)


def argument_product(table, in_idx, a_idx, s_idx, beta, gamma, pad_row):
    """Z[0 ... n] of one argument as residues: `table` the residues of the argument's compressed table, the three index columns
    over the same n rows."""
    n = len(in_idx)
    rows = [row_of_index(c).tolist() for c in (in_idx, a_idx, s_idx)]
    tab = table_column(n, pad_row).tolist()
    z, out = 1, [1]
    for i, t, a, s in zip(rows[0], tab, rows[1], rows[2]):
        f = (table[i] + beta) * (table[t] + gamma) % R * inv((table[a] + beta) % R) % R * inv((table[s] + gamma) % R) % R
        z = z * f % R
        out.append(z)
    return out


def grand_product(tables_fr, inputs, a, s, beta, gamma, pad_row, rows=None):
    """[n_sets][5] lists Z[0 ... rows] of residues, from int [n_sets, 5, >= rows] index columns (rows: default all they hold)."""
    inputs, a, s = np.asarray(inputs), np.asarray(a), np.asarray(s)
    rows = inputs.shape[2] if rows is None else rows
    tables = [values(t) for t in tables_fr]
    return [[argument_product(tables[TABLE_OF_TAG[tag]], inputs[st, tag - 1, :rows], a[st, tag - 1, :rows], s[st, tag - 1, :rows], beta, gamma, pad_row)
             for tag in TAGS] for st in range(inputs.shape[0])]


def z_cells(z, n_rows, k):
    """(uint8[n_sets, 5, last + 1, 32], uint8[n_sets, 5, 32]): the rows 0 ... last = min(n_rows, 2^k - 1) the device writes and the
    closing cells Z[n_rows], from grand_product's lists (which may run further than n_rows)."""
    last = min(n_rows, (1 << k) - 1)
    col = np.stack([np.stack([cells(arg[:last + 1]) for arg in st]) for st in z])
    closing = np.stack([cells([arg[n_rows] for arg in st]) for st in z])
    return col, closing


def report(z, n_rows):
    """The dict of api.grand_report_dict"""
    opened = [(s, t) for s, st in enumerate(z) for t in TAGS if st[t - 1][n_rows] != 1]
    return {"arguments": 5 * len(z), "open": len(opened), "first_open": min(opened) if opened else None}
