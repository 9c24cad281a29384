"""The case list of tests/test_gpu_circuits.py and the kernel instantiations it launches (imports without a GPU).

The many-circuit kernel lives in its own namespace, aesw_circ, next to the aesw:: kernels whose sweep is
tests/kernel_cases.py.  tests/test_circuits_coverage.py holds every kernel of libaesw.so, in any namespace, against the
union of both lists."""

TABLE_PATHS = ("xtime", "generic")  # the blocks' witness through both table paths of encrypt_kernel

# (K, N, C): K 7 ... 16, N in {1, 3}, C in {1, 3, 37}.  Below K = 11 no block fits a circuit (key rows only).
SHAPES = ((7, 1, 3), (9, 3, 1), (10, 1, 37), (11, 3, 37), (12, 1, 3), (13, 3, 3), (14, 1, 37), (15, 3, 1), (16, 1, 3), (16, 3, 37))


def assemble_kernel(as_fr):
    return "aesw_circ::circuit_assemble_kernel<%s>" % ("true" if as_fr else "false")


def launched():
    """Every instantiation the circuit sweep launches, named as `nm -C` shows them (namespace kept, spaces removed)."""
    out = set()
    for as_fr in (False, True):
        out.add(assemble_kernel(as_fr))
    return out


def ragged_counts(cap, cap0, n_sets, c, rng):
    """C block counts that cover the ragged cases: a circuit of 0 blocks (key rows only), one of exactly the capacity, and a
    last one that ends inside set 1 (inside set 0 when there is no set 1); the others random in 0 ... cap."""
    if cap == 0:
        return [0] * c
    counts = [int(v) for v in rng.integers(0, cap + 1, c)]
    counts[0] = cap if c > 1 else counts[0]
    if c > 2:
        counts[1] = 0
    if n_sets > 1 and cap > cap0:
        counts[-1] = cap0 + max(1, (cap - cap0) // (2 * (n_sets - 1)))
    else:
        counts[-1] = max(1, cap // 2)
    return counts
