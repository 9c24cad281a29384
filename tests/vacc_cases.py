"""The case list of tests/test_gpu_vacc.py and the kernel it launches (imports without a GPU).  The shapes, the ragged adds, the
forced chunks and the contention case are tests/acc_cases.py's: the accumulator's, since the histograms are.
tests/test_vacc_library.py holds every kernel of libaesw_vacc.so against launched()."""
from acc_cases import CONTENTION, FORCED_CHUNKS, LONG_CHUNKS, LONG_FROM, MANY_RUNS, MANY_SETS, MANY_TOUCHED, PACKED, SHAPES, TABLE_SETS, VALUES, ragged  # noqa: F401

# what a miss case corrupts: (name, column, note)
CORRUPTIONS = ("y", "z", "pt", "kz", "y+z")


def launched():
    """Every kernel the sweep launches, named as `nm -C` shows it."""
    return {"aesw_vacc::vacc_count_kernel"}
