"""The case lists of tests/test_gpu_sigma_tables.py, test_gpu_sigma_product.py and test_gpu_sigma_chain.py and the kernels they
launch (imports without a GPU).  tests/test_sigma_library.py holds every kernel of libaesw_sigma.so against launched()."""
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


def seeded(seed):
    import numpy as np
    return int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % R


def launched():
    return {"aesw_sigma::sigma_tables_kernel", "aesw_sigma::sigma_prepare_kernel", "aesw_sigma::sigma_chunk_kernel", "aesw_sigma::sigma_carry_kernel",
            "aesw_sigma::sigma_chain_kernel"} | {"aesw_sigma::sigma_scan_kernel<%d>" % m for m in STORE_MODES}
