"""The case list of tests/test_gpu_vals_check.py and the kernel instantiations of libaesw_vals.so it launches (imports without
a GPU).  tests/test_vals_check_library.py holds every kernel of that library against this list, as
tests/test_cols_check_library.py holds libaesw_cols.so against tests/cols_check_cases.py."""

KEY_MODES = ("shared", "scheduled", "per_block")  # scheduled: the slab aesw_schedule_key_device wrote, d_keys NULL and given
SIZES = (1, 67, 4099, (1 << 16) + 5)
TABLE_SETS = ("reference", "fips", "random")
HEADLINE = 1 << 20  # blocks, per-block keys


def check_kernel(per_block_keys):
    return "aesw_vals::vals_check_kernel<%s>" % ("true" if per_block_keys else "false")


REPORT_INIT = "aesw_vals::vals_report_init_kernel"  # resets the report in front of every check launch


def launched():
    """Every instantiation the sweep launches, named as `nm -C` shows them (namespace kept, spaces removed)."""
    return {check_kernel(m == "per_block") for m in KEY_MODES} | {REPORT_INIT}
