"""The case lists of tests/test_gpu_theta_table.py, test_gpu_theta_inputs.py and test_gpu_theta_columns.py and the kernels they
launch (imports without a GPU).  tests/test_theta_library.py holds every kernel of libaesw_theta.so against launched()."""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of bn256's scalar field
THETA_SEEDS = (0x7468, 0x6574)                 # two seeded random thetas, next to 0, 1 and r - 1
NONCANONICAL = (R, R + 1, (1 << 256) - 1)
# (k, n_sets): the smallest shapes at which the inputs kernel takes another path -- no key rows; the key rows just fit and no
# block does; sets of one block; more than one workgroup per set and blocks that straddle workgroups
INPUT_SHAPES = ((8, 1), (9, 1), (11, 2), (12, 3))
COLUMN_ROWS = (66561, 66563, (1 << 17) - 6, 1 << 17)  # n_rows: the table alone, an odd tail, the usable rows, 2^k
PAD_ROWS = (0, 66560)
STORE_MODES = (0, 1, 2)  # "fr_store_mode": one instantiation of the columns kernel each


def launched():
    return {"aesw_theta::theta_table_kernel", "aesw_theta::theta_inputs_kernel", "aesw_theta::theta_report_kernel"} | \
        {"aesw_theta::theta_columns_kernel<%d>" % m for m in STORE_MODES}
