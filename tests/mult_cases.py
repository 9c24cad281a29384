"""The case list of tests/test_gpu_mult.py and the kernel instantiations it launches (imports without a GPU).
tests/test_mult_library.py holds every kernel of libaesw_mult.so against launched()."""
import circuit_cases as cc

DENSE, PACKED, VALUES = 0, 1, 2
LAYOUTS = (DENSE, PACKED)
FORM_AUTO, FORM_DIRECT, FORM_PRIVATE = 0, 1, 2
FORMS = (FORM_DIRECT, FORM_PRIVATE)
TABLE_SETS = ("reference", "random")  # the context's runtime tables: the reference's, and one set that is no xtime set
SHAPES = cc.SHAPES                    # (K, N, C) of the many-circuit sweep, with cc.ragged_counts

# every block identical, so that all lanes of all waves hit the same bins: (K, N, C, blocks per circuit or None = capacity)
CONTENTION = ((23, 1, 1, None), (16, 3, 37, None))


def kernel(form, layout):
    return "aesw_mult::mult_%s_kernel<%d>" % ("direct" if form == FORM_DIRECT else "private", layout)


def launched():
    """Every instantiation the sweep launches, named as `nm -C` shows them."""
    return {kernel(f, lay) for f in FORMS for lay in LAYOUTS} | {"aesw_mult::mult_init_kernel"}
