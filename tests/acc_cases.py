"""The case list of tests/test_gpu_acc.py and the kernel instantiations it launches (imports without a GPU).
tests/test_acc_library.py holds every kernel of libaesw_acc.so against launched()."""
DENSE, PACKED, VALUES = 0, 1, 2
LAYOUTS = (DENSE, PACKED)
TABLE_SETS = ("reference", "fips")  # the context's runtime tables

# (K, N, blocks): one and three sets; a partly filled last set (K = 12 holds 1 + 3 blocks); the key rows' boundary, where no
# block fits (K = 9: the key slab counts, K = 8: it does not); two full sets of 46 and 48 blocks (K = 16), the smallest K at which a
# wave of a workgroup makes five trips or more through the staging loop: 46 = 5 x 8 + 6 = 7 x 6 + 4, 48 = 6 x 8 = 8 x 6
SHAPES = ((14, 1, 10), (14, 3, 34), (12, 2, 3), (9, 1, 0), (8, 1, 0), (16, 2, 94))
RAGGED = (1, 7, 16)           # the lengths of the ragged adds, then the rest: 1 + 7 + 16 + 10 of 34 blocks crosses both set boundaries
FORCED_CHUNKS = (1, 2, 5, 0)  # blocks per pair of workgroups; 0: the default rule
LONG_CHUNKS = (17, 40)        # for shapes of LONG_FROM blocks or more: chunks longer than one round of the waves (17: three trips for the first
LONG_FROM = 64                # wave, two for the rest; 40: five rounds, then a last chunk of 6 or 8 blocks, no more than there are waves)
CONTENTION = (14, 3, 34, 2)   # every block identical, K, N, blocks, chunk: 18 pairs of workgroups add into the same few hundred words
# as many sets as a call accepts: K = 12 / N = 1024 holds 1 + 1023 x 3 = 3 070 blocks.  (first block, count) of four adds after one
# reset: set 0; set 1, whole; the last two blocks of set 511 and the first two of set 512; the last two of set 1021 and all of sets
# 1022 and 1023 -- seven sets touched by 16 blocks, 1 017 left alone
MANY_SETS = (12, 1024)
MANY_RUNS = ((0, 1), (1, 3), (1532, 4), (3062, 8))
MANY_TOUCHED = (0, 1, 511, 512, 1021, 1022, 1023)


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
