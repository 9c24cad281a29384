"""The case lists of tests/test_gpu_sigma_tables.py, test_gpu_sigma_product.py, test_gpu_sigma_reach.py and test_gpu_sigma_chain.py,
the synthetic columns and mappings they run over, and the kernels they launch (imports without a GPU).
tests/test_sigma_library.py holds every kernel of libaesw_sigma.so against launched()."""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of bn256's scalar field
CHALLENGE_SEEDS = (0x7362, 0x7367)     # beta, gamma
NONCANONICAL = (R, (1 << 256) - 1)
TABLE_KS = (10, 14, 15, 17)            # below, at and above the split of omega's exponent at bit 14
TABLE_COLS = (1, 5, 14)
# (k, n_cols, chunk_len, n_rows): k 10, 11, 12 -- one chunk of 1 024 rows, two, several; a short last set and set chains of every
# length that matters; n_rows 1, around a chunk's end, the usable rows 2^k - 6 and 2^k (no room for Z[n_rows]).  One pairing, not
# the cross product.
PRODUCTS = (
    (10, 1, 1, 1),
    (10, 3, 3, 1023),
    (10, 4, 3, 1024),
    (11, 5, 2, 1025),
    (11, 4, 3, 1024),            # the second chunk holds the closing row alone
    (11, 7, 3, (1 << 11) - 6),
    (12, 14, 3, 1 << 12),
    (12, 9, 8, (1 << 12) - 6),
    (12, 3, 3, 1),
)
STORE_MODES = (0, 1, 2)                # "fr_store_mode": one instantiation of the scan kernel each
STORE_SHAPE = (11, 7, 3, (1 << 11) - 6)
ZERO_SHAPE = (12, 7, 3, (1 << 12) - 6)  # sets 0-2, 3-5, 6
ZERO_CELL = (4, 1024 + 301)            # (column, row): set 1, its second chunk, inside a lane
CHAIN = (17, 2, 150, 3)                # K, N, blocks, chunk_len: the shape of tests/test_gpu_grand_chain.py

# tests/test_gpu_sigma_reach.py: what the lists above never make a kernel do.
# Many sets: sigma_chain_kernel scans them 256 a turn, a set a thread.  300 sets: four full waves and a second turn of 44 (and two
# workgroups of sigma_prepare_kernel); 66 sets, the last of one column: one full wave and two lanes of the next.
MANY_SETS = ((10, 300, 1, 1018), (10, 131, 2, 1018))
MANY_SETS_ZEROS = ((70, 517), (260, 300))  # (set, row) of two planted zero terms of the 300-set shape: the second wave, the second turn
# Many chunks: sigma_carry_kernel scans a set's chunks 256 a turn.  256 chunks: one turn that ends on the loop's bound (and
# n_rows = 2^k); 257 chunks in two sets, the second short: the upwards scan's second turn holds chunk 256 and the downwards scan's
# chunk 0, `set * stride` with a stride of 512, and rows at and above 2^14 read every cell of the high power table.
MANY_CHUNKS = ((18, 1, 1, 1 << 18), (19, 3, 2, (1 << 18) + 5))
MANY_CHUNKS_ZEROS = ((0, (1 << 18) + 1), (1, 3 * 1024 + 517))  # (column, row), both in set 0 of the 257-chunk shape: chunk 256, chunk 3
ZERO_TARGET = (0, 2000)                # (column, row) of the cell every planted entry of ZERO_EDGES maps to
# name -> the planted (column, row)s of ZERO_SHAPE, whose lanes own four rows and whose chunks 1 024
ZERO_EDGES = {
    "two_in_a_lane": ((4, 1324 + 1), (5, 1324 + 3)),       # rows q = 1 and q = 3 of one lane of set 1
    "a_lanes_first_row": ((4, 1328),),
    "a_chunks_last_and_next_first": ((3, 2047), (5, 2048)),
    "row_0_of_set_0": ((1, 0),),                           # only Z_0[0] is left
    "the_last_row_of_the_last_set": ((6, (1 << 12) - 7),),  # only the last closing cell is zero
    "two_sets": ((3, 700), (6, 100)),
}


def seeded(seed):
    import numpy as np
    return int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % R


def world(k, n_cols, n_rows, seed):
    """(buffers uint8 [n_cols, 2^k] in buffer order, source, columns in permutation order, mapping uint32 [n_cols, 2^k]): the
    mapping a random partition of the cells in the rows below n_rows into cycles, bytes constant on each cycle, the identity at
    and above n_rows -- so the product closes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = 1 << k
    cells = (np.arange(n_cols)[:, None] * n + np.arange(n_rows)[None, :]).reshape(-1)
    perm = rng.permutation(cells)
    starts = rng.random(len(perm)) < 0.4
    starts[0] = True
    at = np.arange(len(perm))
    seg_start = np.maximum.accumulate(np.where(starts, at, 0))
    nxt = at + 1
    last = np.append(starts[1:], True)
    nxt[last] = seg_start[last]
    mapping = np.arange(n_cols * n, dtype=np.uint32)
    mapping[perm] = perm[nxt]
    seg_bytes = rng.integers(0, 256, len(perm), dtype=np.uint8)
    columns = rng.integers(0, 256, n_cols * n, dtype=np.uint8)
    columns[perm] = seg_bytes[seg_start]
    columns, mapping = columns.reshape(n_cols, n), mapping.reshape(n_cols, n)
    source = rng.permutation(n_cols).astype(np.uint32)
    buffers = np.empty_like(columns)
    buffers[source] = columns  # permutation column c lies in buffer source[c]
    return buffers, source, columns, mapping


def planted_zeros(k, w, cells, target, beta):
    """(buffers, source, columns, mapping, gamma): the world `w` with a zero denominator at every (column, row) of `cells` and, for
    all that is likely, nowhere else.  Neither the kernels nor the model need the mapping to be a permutation: every planted cell
    gets one byte v and maps to the cell `target` (column, row), and gamma = -(v + beta * label(target)).  v is not the target's
    byte, so the numerator at the target -- and the denominator of the cell in front of it on its cycle, which shares its byte --
    stays non-zero.  The argument no longer closes."""
    import numpy as np
    _buffers, source, columns, mapping = w
    assert target not in cells
    columns, mapping = columns.copy(), mapping.copy()
    v = (int(columns[target]) + 1) & 255
    for cell in cells:
        columns[cell] = v
        mapping[cell] = (target[0] << k) + target[1]
    buffers = np.empty_like(columns)
    buffers[source] = columns
    label = pow(pow(7, 1 << 28, R), target[0], R) * pow(pow(7, (R - 1) >> k, R), target[1], R) % R  # delta^column * omega^row
    return buffers, source, columns, mapping, (-(v + beta * label)) % R


def launched():
    return {"aesw_sigma::sigma_tables_kernel", "aesw_sigma::sigma_prepare_kernel", "aesw_sigma::sigma_chunk_kernel", "aesw_sigma::sigma_carry_kernel",
            "aesw_sigma::sigma_chain_kernel"} | {"aesw_sigma::sigma_scan_kernel<%d>" % m for m in STORE_MODES}
