"""The case list of tests/test_gpu_circ_check.py and the kernel instantiations of libaesw_circ.so it launches (imports without
a GPU).  tests/test_circ_check_library.py holds every kernel of that library against this list, as
tests/test_circuits_coverage.py holds libaesw.so against tests/kernel_cases.py and tests/circuit_cases.py."""
import circuit_cases as cc

DENSE, PACKED = 0, 1
LAYOUTS = (DENSE, PACKED)
SHAPES = cc.SHAPES  # (K, N, C) of the many-circuit assemble sweep: the batches the checker certifies


def check_kernel(layout):
    return "aesw_circ::circ_check_kernel<%d>" % layout


REPORT_INIT = "aesw_circ::circ_report_init_kernel"  # resets the report in front of every check launch


def launched():
    """Every instantiation the sweep launches, named as `nm -C` shows them (namespace kept, spaces removed)."""
    return {check_kernel(layout) for layout in LAYOUTS} | {REPORT_INIT}
