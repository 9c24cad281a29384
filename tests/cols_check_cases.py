"""The case list of tests/test_gpu_cols_check.py and the kernel instantiations of libaesw_cols.so it launches (imports without
a GPU).  tests/test_cols_check_library.py holds every kernel of that library against this list, as
tests/test_circ_check_library.py holds libaesw_circ.so against tests/circ_check_cases.py."""

FORMS = (False, True)  # as_fr
# (K, N, counts or None for "full capacity", C): the batches of Context.circuits the checker certifies
SHAPES = ((11, 1, 3), (12, 2, 5), (14, 1, 64), (16, 3, 2))
SLAB_LAYOUTS = (0, 1)  # the columns are assembled from DENSE and from PACKED slabs


def check_kernel(as_fr):
    return "aesw_cols::cols_check_kernel<%s>" % ("true" if as_fr else "false")


REPORT_INIT = "aesw_cols::cols_report_init_kernel"  # resets the report in front of every check launch


def launched():
    """Every instantiation the sweep launches, named as `nm -C` shows them (namespace kept, spaces removed)."""
    return {check_kernel(f) for f in FORMS} | {REPORT_INIT}


def counts(pkg, k, n_sets, nc):
    """Blocks per circuit of a shape: K=11 N=1 an empty circuit among three, K=12 ragged, K=14 64 circuits of every fill,
    K=16 N=3 every circuit at full capacity."""
    cap = pkg.block_capacity(k, n_sets)
    if k == 11:
        return [cap, 0, max(cap - 1, 0)][:nc]
    if k == 16:
        return [cap] * nc
    return [(7 * c + 3) % (cap + 1) for c in range(nc)]
