"""The case lists of tests/test_gpu_grand_invert.py, test_gpu_grand_product.py, test_gpu_grand_reach.py and test_gpu_grand_chain.py and the kernels they
launch (imports without a GPU).  tests/test_grand_library.py holds every kernel of libaesw_grand.so against launched()."""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of bn256's scalar field
THETA_SEED = 0x7468                            # the theta of every table these tests invert
CHALLENGE_SEEDS = (0x6265, 0x6761)             # two seeded random challenges, next to 0, 1 and r - 1
NONCANONICAL = (R, (1 << 256) - 1)
ZERO_TERM_ROW = 40000                          # beta = -T_1[this row]: the one planted zero term of the invert test
PRODUCT_ROWS = (66561, 66563, (1 << 17) - 6, 1 << 17)  # n_rows: the table alone, an odd tail, the usable rows, 2^k (no room for Z[n_rows])
PAD_ROWS = (0, 66560)
STORE_MODES = (0, 1, 2)  # "fr_store_mode": one instantiation of the scan kernel each
K = 17                   # the smallest k that holds the table
# tests/test_gpu_grand_reach.py: (k, n_sets, n_rows, pad_row).  grand_carry_kernel scans an argument's chunks 256 a turn, and k = 17
# has 128 of them: 2^18 + 3 rows are 257 chunks, the smallest number whose second turn holds a chunk.
MANY_CHUNKS = (19, 1, (1 << 18) + 3, 66560)
MANY_CHUNKS_SEED = 0x6733


def seeded(seed):
    import numpy as np
    return int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % R


def launched():
    return {"aesw_grand::grand_invert_kernel", "aesw_grand::grand_invert_report_kernel", "aesw_grand::grand_chunk_kernel",
            "aesw_grand::grand_carry_kernel", "aesw_grand::grand_report_kernel"} | {"aesw_grand::grand_scan_kernel<%d>" % m for m in STORE_MODES}
