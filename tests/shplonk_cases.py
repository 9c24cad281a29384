"""The case lists of tests/test_shplonk_model.py, test_gpu_shplonk_columns.py, test_gpu_shplonk_reach.py and test_gpu_shplonk_chain.py,
and the kernels they launch (imports without a GPU).  tests/test_shplonk_library.py holds every kernel of libaesw_shplonk.so
against launched()."""
import functools

import ntt_model as nm
import open_model as om

KS = (10, 11)            # one chunk; two chunks, so the carry is crossed
STORE_MODES = (0, 1, 2)  # "fr_store_mode": one instantiation of the combine and of the scan kernel each
REACH_K = 19             # the smallest k whose carry takes a second turn (open_cases.REACH_K)
CHAIN_ROTATIONS = (0, 1, -1)
# (point indices, columns): t = 1, 2, 3 and 8, m = 5 and 1; the super set is points(k): 0, 1, omega_k, r - 1 and four seeded values
SETS = (((4,), 5), ((0, 1), 1), ((2, 3, 5), 1), ((0, 1, 2, 3, 4, 5, 6, 7), 5))
NAMESPACE = "aesw_shplonk"


class Plan:
    """the shape of api.MultiopenPlan, for the model and the driver where no package is at hand"""

    def __init__(self, rotations, sets):
        self.rotations, self.sets = list(rotations), [(tuple(idx), list(cols)) for idx, cols in sets]
        self.set_points = [len(idx) for idx, _cols in self.sets]
        self.set_cols = [len(cols) for _idx, cols in self.sets]
        self.point_index = [p for idx, _cols in self.sets for p in idx]

    def text(self):
        """what tests/shplonk_driver.cpp reads"""
        return "%d %d\n" % (len(self.rotations), len(self.sets)) + "".join("%d %d %s\n" % (len(idx), len(cols), " ".join(map(str, idx))) for idx, cols in self.sets)


def points(k, seed=0x7368):
    return [0, 1, nm.omega(k), nm.R - 1] + nm.seeded_values(4, seed + k)


def plan(sets=SETS):
    """column ids count up through the sets"""
    out, first = [], 0
    for idx, m in sets:
        out.append((idx, list(range(first, first + m))))
        first += m
    return Plan(range(8), out)


@functools.lru_cache(maxsize=None)
def stage(k, sets=SETS, wrong=None):
    """(plan, points, columns, evals, y, v, u) in plain values: seeded columns, their own evaluations -- but for evaluation
    `wrong` = (set, column, point), which is one more than the column's"""
    p, pts = plan(sets), points(k)
    columns = [[nm.seeded_values(1 << k, 0x7363 + 64 * k + c) for c in cols] for _idx, cols in p.sets]
    evals = [[[om.evaluate(column, pts[q]) for q in idx] for column in columns[i]] for i, (idx, _cols) in enumerate(p.sets)]
    if wrong is not None:
        i, j, s = wrong
        evals[i][j][s] = (evals[i][j][s] + 1) % nm.R
    y, v, u = nm.seeded_values(3, 0x797675 + k)
    return p, pts, columns, evals, y, v, u


def flat_evals(evals):
    """d_evals: set by set, column by column, point by point"""
    return [e for of_set in evals for of_column in of_set for e in of_column]


def launched():
    return {"%s::shplonk_%s_kernel" % (NAMESPACE, name) for name in ("prepare", "finish", "powers", "chunk", "carry", "report")} | \
        {"%s::shplonk_%s_kernel<%d>" % (NAMESPACE, name, m) for name in ("combine", "scan") for m in STORE_MODES}
