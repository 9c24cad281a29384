"""The case lists of tests/test_gpu_ntt_transform.py, test_gpu_ntt_reach.py and test_gpu_ntt_chain.py, and the kernels they launch
(imports without a GPU).  tests/test_ntt_library.py holds every kernel of libaesw_ntt.so against launched()."""
PASS_LOG = 10                          # csrc/aesw_ntt.h's NTT_PASS_LOG; tests/test_ntt_model.py holds the two equal
P = PASS_LOG
# the transform sizes of the full-column sweep: one pass; a second pass of one stage; two full passes and the first k of three
# passes where a Python model run can still follow (it cannot: 2 P = 20 is above 18, so those are test_gpu_ntt_reach.py's)
KS = tuple(k for k in (10, P + 1, 2 * P, 2 * P + 1) if k <= 18)
# (k, n_cols): one shape has three columns
SHAPES = tuple((k, 3 if k == P + 1 else 1) for k in KS)
# (k, ext_k, zeta_sel, n_cols): ext_k - k in {0, 1, 3}, both zetas, one-pass and two-pass extended sizes
EXTENDED = ((10, 10, 1, 1), (10, 11, 0, 3), (10, 13, 1, 1), (11, 12, 1, 2))
STORE_MODES = (0, 1, 2)                # "fr_store_mode": one instantiation of the pass kernel each
TABLES_MAX_K = 20                      # tables built once for 2^20 serve k = 10 and k = 17
TABLES_KS = (10, 17)
THREE_PASSES = 2 * P + 1               # 21: the smallest k with three passes; no model run reaches it
BIG = (22, 33)                         # (k, n_cols): 33 * 2^22 cells of 32 bytes pass 4 GiB per buffer
CHAIN = (17, 2, 150, 19)               # K, N, blocks, ext_k: the shape of tests/test_gpu_grand_chain.py


def launched():
    return {"aesw_ntt::ntt_tables_kernel"} | {"aesw_ntt::ntt_pass_kernel<%d>" % m for m in STORE_MODES}
