"""halo2's permutation argument restated in Python integers (plonk/permutation/prover.rs::commit and
permutation/keygen.rs::Assembly::copy of halo2_proofs v0.3.0, as include/aesw_sigma.h states them), with no line shared with
csrc/aesw_sigma.h or csrc/aesw_fr.h: the constants derived from the generator 7, a per-row factor with inv(0) = 0, the last_z chain
across sets, Assembly.copy over cell indices and the column order of a FixedAes128Config circuit.  Held against the header in
tests/test_sigma_model.py; the yardstick of the tests/test_gpu_sigma_*.py."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
M = 1 << 256
M_INV = pow(M, -1, R)
G = 7                 # halo2curves' MULTIPLICATIVE_GENERATOR of bn256's scalar field
S = 28                # r - 1 = 2^28 * t
T = (R - 1) >> S
DELTA = pow(G, 1 << S, R)
ONE_CELL = (M % R).to_bytes(32, "little")
NONE = 0xFFFFFFFFFFFFFFFF
SPLIT = 14


def omega(k):
    return pow(G, (R - 1) >> k, R)


def inv(x):
    return pow(x, R - 2, R) if x else 0


def cells(residues):
    """uint8[n, 32]: the Montgomery cells of residues"""
    return np.frombuffer(b"".join((v * M % R).to_bytes(32, "little") for v in residues), np.uint8).reshape(-1, 32)


def values(cell_bytes):
    raw = np.ascontiguousarray(cell_bytes, np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") * M_INV % R for row in raw]


def tables(k, n_cols):
    """The residues of the power tables in the order of d_tables: omega^j, omega^(j * 2^14), delta^c."""
    w = omega(k)
    return [pow(w, j, R) for j in range(1 << min(k, SPLIT))] + [pow(w, j << SPLIT, R) for j in range(1 << max(k - SPLIT, 0))] + \
        [pow(DELTA, c, R) for c in range(n_cols)]


def sets_of(n_cols, chunk_len):
    """[(first column, end column)] of every set"""
    return [(c, min(c + chunk_len, n_cols)) for c in range(0, n_cols, chunk_len)]


def label(k, w_pows, d_pows, m):
    return d_pows[m >> k] * w_pows[m & ((1 << k) - 1)] % R


def row_terms(k, columns, mapping, beta, gamma, chunk_len, rows):
    """[set] -> (num[i], den[i]) for the rows in `rows` (an iterable): columns a list of byte sequences (None: zero bytes), mapping
    int [n_cols][2^k]; an entry at or above n_cols * 2^k reads as the cell itself."""
    n_cols, n = len(columns), 1 << k
    w = omega(k)
    d_pows = [pow(DELTA, c, R) for c in range(n_cols)]
    rows = list(rows)
    w_at = {}

    def w_pow(i):
        if i not in w_at:
            w_at[i] = pow(w, i, R)
        return w_at[i]
    out = []
    for first, end in sets_of(n_cols, chunk_len):
        nums, dens = [], []
        for i in rows:
            num = den = 1
            for c in range(first, end):
                v = int(columns[c][i]) if columns[c] is not None else 0
                m = int(mapping[c][i])
                if m >= n_cols * n:
                    m = c * n + i
                num = num * (v + beta * d_pows[c] % R * w_pow(i) + gamma) % R
                den = den * (v + beta * d_pows[m >> k] % R * w_pow(m & (n - 1)) + gamma) % R
            nums.append(num)
            dens.append(den)
        out.append((nums, dens))
    return out


def product(k, columns, mapping, beta, gamma, chunk_len, n_rows):
    """([set] -> Z[0 ... n_rows] residues, report dict): the literal chain, one inverse per row, Z_{s+1}[0] = Z_s[n_rows].  A beta or
    gamma that is not canonical: every cell zero, the report says so."""
    n_cols, n = len(columns), 1 << k
    n_sets = len(sets_of(n_cols, chunk_len))
    out_of_range = sum(1 for c in range(n_cols) for i in range(n_rows) if int(mapping[c][i]) >= n_cols * n)
    if not (0 <= beta < R and 0 <= gamma < R):
        return [[0] * (n_rows + 1) for _ in range(n_sets)], {"sets": n_sets, "open": True, "zero_terms": 0, "first_zero": None, "out_of_range": out_of_range,
                                                               "noncanonical": True}
    z, last, zeros = [], 1, []
    for s, (nums, dens) in enumerate(row_terms(k, columns, mapping, beta, gamma, chunk_len, range(n_rows))):
        col = [last]
        for i, (num, den) in enumerate(zip(nums, dens)):
            if den == 0:
                zeros.append(s * n + i)
            col.append(col[-1] * num % R * inv(den) % R)
        z.append(col)
        last = col[n_rows]
    return z, {"sets": n_sets, "open": last != 1, "zero_terms": len(zeros), "first_zero": min(zeros) if zeros else None, "out_of_range": out_of_range,
               "noncanonical": False}


def product_batched(k, columns, mapping, beta, gamma, chunk_len, n_rows):
    """product() for the shapes it is too slow for (tests/test_sigma_model.py holds the two equal): the same arguments, the same
    return value.  The powers of omega and of delta are running products, and a set's denominators are inverted together by
    Montgomery's trick -- the prefix products of the non-zero ones, one pow, one walk back; a zero denominator is left out of
    the prefixes and gets the inverse 0."""
    n_cols, n = len(columns), 1 << k
    sets = sets_of(n_cols, chunk_len)
    here = np.arange(n_rows, dtype=np.int64)
    images, out_of_range = [], 0
    for c in range(n_cols):
        m = np.asarray(mapping[c][:n_rows]).astype(np.int64) & 0xFFFFFFFF
        outside = m >= n_cols * n
        out_of_range += int(outside.sum())
        images.append(np.where(outside, c * n + here, m))
    if not (0 <= beta < R and 0 <= gamma < R):
        return [[0] * (n_rows + 1) for _ in sets], {"sets": len(sets), "open": True, "zero_terms": 0, "first_zero": None, "out_of_range": out_of_range,
                                                    "noncanonical": True}
    w, w_pows, acc = omega(k), [], 1
    for _ in range(n):
        w_pows.append(acc)
        acc = acc * w % R
    bd, acc = [], beta
    for _ in range(n_cols):
        bd.append(acc)
        acc = acc * DELTA % R
    z, last, zeros = [], 1, []
    for s, (first, end) in enumerate(sets):
        nums, dens = [1] * n_rows, [1] * n_rows
        for c in range(first, end):
            v = np.asarray(columns[c][:n_rows]).astype(np.int64).tolist() if columns[c] is not None else [0] * n_rows
            m_col, m_row = (images[c] >> k).tolist(), (images[c] & (n - 1)).tolist()
            b = bd[c]
            for i in range(n_rows):
                vg = v[i] + gamma
                nums[i] = nums[i] * (vg + b * w_pows[i]) % R
                dens[i] = dens[i] * (vg + bd[m_col[i]] * w_pows[m_row[i]]) % R
        prefix, acc = [], 1  # prefix[i]: the product of the non-zero denominators below row i
        for d in dens:
            prefix.append(acc)
            if d:
                acc = acc * d % R
        back = pow(acc, R - 2, R)  # the inverse of the product of the non-zero denominators at and above the row the walk is at
        inverses = [0] * n_rows
        for i in range(n_rows - 1, -1, -1):
            if dens[i]:
                inverses[i] = back * prefix[i] % R
                back = back * dens[i] % R
            else:
                zeros.append(s * n + i)
        col = [last]
        for num, inverse in zip(nums, inverses):
            last = last * num % R * inverse % R
            col.append(last)
        z.append(col)
    return z, {"sets": len(sets), "open": last != 1, "zero_terms": len(zeros), "first_zero": min(zeros) if zeros else None, "out_of_range": out_of_range,
               "noncanonical": False}


def z_cells(z, n_rows, k):
    """(uint8[S, last + 1, 32], uint8[S, 32]): the rows the device writes and the closing cells"""
    last = min(n_rows, (1 << k) - 1)
    return np.stack([cells(col[:last + 1]) for col in z]), cells([col[n_rows] for col in z])


# ---- keygen ----------------------------------------------------------------------------------------------------------------------

def columns(n_sets):
    return 3 * n_sets + 2


def sources(n_sets):
    """x0 y0 z0 words rcon x1 y1 z1 ...: the assembled advice column of each permutation column (3 n_sets + 1: the fixed one)"""
    return [0, 1, 2, 3 * n_sets, 3 * n_sets + 1] + list(range(3, 3 * n_sets))


def column_of_advice(n_sets, a):
    return sources(n_sets).index(a)


class Assembly:
    """permutation::keygen::Assembly over cell indices c * 2^k + i"""

    def __init__(self, cells_):
        self.mapping = list(range(cells_))
        self.aux = list(range(cells_))
        self.sizes = [1] * cells_

    def copy(self, left, right):
        if self.aux[left] == self.aux[right]:
            return
        if self.sizes[self.aux[left]] < self.sizes[self.aux[right]]:
            left, right = right, left
        head, other = self.aux[left], self.aux[right]
        self.sizes[head] += self.sizes[other]
        i = right
        while True:
            self.aux[i] = head
            i = self.mapping[i]
            if i == right:
                break
        self.mapping[left], self.mapping[right] = self.mapping[right], self.mapping[left]


def placed_edges(k, n_sets, n_blocks, key_edges, block_edges, placement):
    """[(dst cell, src cell)] of every copy_advice() in synthesize()'s call order: the key schedule, then every block.  The edges are
    the structured arrays of api.key_copy_graph / block_copy_graph, placement(b) -> (set, first row)."""
    n = 1 << k

    def cell(space, col, row, st, first):
        advice = 3 * st + col if space == 0 else col if space == 1 else 3 * n_sets
        return column_of_advice(n_sets, advice) * n + (first + row if space == 0 else row)
    out = []
    for edges, places in ((key_edges, [(0, 0)]), (block_edges, [placement(b) for b in range(n_blocks)])):
        for st, first in places:
            for e in edges:
                out.append((cell(int(e["dst_space"]), int(e["dst_col"]), int(e["dst_row"]), st, first),
                            cell(int(e["src_space"]), int(e["src_col"]), int(e["src_row"]), st, first)))
    return out


def mapping(k, n_sets, edges):
    """uint32 [3 n_sets + 2, 2^k] from placed_edges: copy(left = the new cell, right = the copied one) in order"""
    a = Assembly(columns(n_sets) << k)
    for dst, src in edges:
        a.copy(dst, src)
    return np.array(a.mapping, np.uint32).reshape(columns(n_sets), 1 << k)


def closing_ratio(k, cols, mapping_, beta, gamma, n_rows):
    """prod num / prod den over every column and every row below n_rows, with one pow: 1 exactly when the argument closes (no zero
    term assumed).  Vectorised over Python-integer object arrays."""
    n_cols, n = len(cols), 1 << k
    w = omega(k)
    w_pows = np.empty(n, object)
    acc = 1
    for i in range(n):
        w_pows[i] = acc
        acc = acc * w % R
    num = den = 1
    for c in range(n_cols):
        v = np.asarray(cols[c][:n_rows]).astype(object)
        m = np.asarray(mapping_[c][:n_rows]).astype(np.int64)
        bd = np.array([beta * pow(DELTA, cc, R) % R for cc in range(n_cols)], object)
        nt = (v + bd[c] * w_pows[:n_rows] + gamma) % R
        dt = (v + bd[m >> k] * w_pows[m & (n - 1)] + gamma) % R
        for t in nt:
            num = num * t % R
        for t in dt:
            den = den * t % R
    return num * inv(den) % R
