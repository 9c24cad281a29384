"""The case list of tests/test_gpu_perm.py and the kernels it launches (imports without a GPU).  tests/test_perm_library.py holds
every kernel of libaesw_perm.so against launched()."""
US = (66561, 66562, 66563, 66564, (1 << 17) - 6, 1 << 17)  # the u % 4 tails, no pad copy at all, u == 2^k
PAD_ROWS = (0, 66560)
GATHER_CELLS = (1, 127, 128, 129, (1 << 17) + 5)
STORE_MODES = (0, 1, 2)  # "fr_store_mode": one instantiation of the gather each


def launched():
    return {"aesw_perm::perm_scan_kernel", "aesw_perm::perm_expand_kernel"} | {"aesw_perm::perm_gather_fr_kernel<%d>" % m for m in STORE_MODES}
