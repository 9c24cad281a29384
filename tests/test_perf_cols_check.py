"""The byte form of the column checker against the slab checker on DENSE slabs of the same batch (tools/cols_bench.py's
method: one process, alternating, median of five): both stage a DENSE image per block and run the same walk, the column form
adds the zero sweep and the strided key rows, so it is expected within 1.25 x.  Marker perf: not part of -m gpu.

First measurement (profiles/cols/README.md, one MI355X): K=20 N=5 C=4  65.6 us against 53.2 us = 1.233 (holds);
K=14 N=1 C=4096  139.3 us against 106.7 us = 1.306: that case MISSES the bound and fails.  The bound stays as set."""
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.perf
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))


@pytest.mark.parametrize("k,n_sets,nc", [(20, 5, 4), (14, 1, 4096)])
def test_byte_form_within_a_quarter_of_the_slab_check(pkg, ctx, k, n_sets, nc):
    import cols_bench
    r = cols_bench.measure(pkg, ctx, k, n_sets, nc)
    print(r)
    assert r["bytes_over_slab"] <= 1.25, r
