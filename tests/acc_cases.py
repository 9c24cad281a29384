"""The case list of tests/test_gpu_acc.py and the kernel instantiations it launches (imports without a GPU).
tests/test_acc_library.py holds every kernel of libaesw_acc.so against launched()."""
DENSE, PACKED, VALUES = 0, 1, 2
LAYOUTS = (DENSE, PACKED)
TABLE_SETS = ("reference", "fips")  # the context's runtime tables

# (K, N, blocks): one and three sets; a partly filled last set (K = 12 holds 1 + 3 blocks); the key rows' boundary, where no
# block fits (K = 9: the key slab counts, K = 8: it does not)
SHAPES = ((14, 1, 10), (14, 3, 34), (12, 2, 3), (9, 1, 0), (8, 1, 0))
RAGGED = (1, 7, 16)           # the lengths of the ragged adds, then the rest: 1 + 7 + 16 + 10 of 34 blocks crosses both set boundaries
FORCED_CHUNKS = (1, 2, 5, 0)  # blocks per pair of workgroups; 0: the default rule
CONTENTION = (14, 3, 34, 2)   # every block identical, K, N, blocks, chunk: 18 pairs of workgroups add into the same few hundred words


def ragged(n):
    """[(first, count)] of RAGGED clipped to n blocks, and the rest."""
    out, at = [], 0
    for length in RAGGED + (n,):
        length = min(length, n - at)
        if length > 0:
            out.append((at, length))
            at += length
    return out


def kernel(name, layout=None):
    return "aesw_acc::acc_%s_kernel" % name + ("" if layout is None else "<%d>" % layout)


def launched():
    """Every instantiation the sweep launches, named as `nm -C` shows them."""
    return {kernel(n, lay) for n in ("add", "key") for lay in LAYOUTS} | {kernel("reset")}
