"""The case lists of tests/test_open_model.py, test_gpu_open_columns.py, test_gpu_open_reach.py and test_gpu_open_chain.py, and the
kernels they launch (imports without a GPU).  tests/test_open_library.py holds every kernel of libaesw_open.so against launched()."""
import ntt_model as nm

CHUNK = 1024                           # csrc/aesw_open.h's OPEN_CHUNK; tests/test_open_model.py holds the two equal
TURN = 256                             # ... and OPEN_TURN: chunks the carry kernel scans at a time
# (k, n_cols, n_points): one chunk; a carry across two chunks, and the column and point strides
SHAPES = ((10, 1, 1), (11, 3, 3))
STORE_MODES = (0, 1, 2)                # "fr_store_mode": one instantiation of the scan and of the fold kernel each
REACH_K = 19                           # the smallest k whose carry takes a second turn: 2^19 / CHUNK = 2 * TURN chunks
CHAIN = (17, 2, 150)                   # K, N, blocks: the shape of tests/test_gpu_ntt_chain.py
assert (1 << REACH_K) // CHUNK == 2 * TURN


def points(k, seed):
    """the points every shape is held at: 0, 1, omega_k, r - 1 and two seeded values"""
    return [0, 1, nm.omega(k), nm.R - 1] + nm.seeded_values(2, seed)


def launched():
    return {"aesw_open::open_powers_kernel", "aesw_open::open_chunk_kernel", "aesw_open::open_carry_kernel"} | \
        {"aesw_open::open_%s_kernel<%d>" % (name, m) for name in ("scan", "fold") for m in STORE_MODES}
