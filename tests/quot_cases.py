"""The case lists of tests/test_gpu_quot_sigma.py and tests/test_quot_model.py, and the kernels the GPU tests launch (imports
without a GPU).  tests/test_quot_library.py holds every kernel of libaesw_quot.so against launched()."""
SIGMA_FR = ((10, 5), (15, 5))          # (k, n_cols): one below and one above the 14-bit split of the power tables
DRIVER = (10, 12, 1, 2, 3, 6)          # the CPU driver's run of the fold: k, ext_k, zeta_sel, n_sets, chunk_len, rows not usable


def launched():
    return {"aesw_quot::quot_sigma_kernel"}
