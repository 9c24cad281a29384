"""The case lists of tests/test_shplonk_model.py, test_gpu_shplonk_columns.py, test_gpu_shplonk_extents.py, test_gpu_shplonk_reach.py and
test_gpu_shplonk_chain.py, and the kernels they launch (imports without a GPU).  tests/test_shplonk_library.py holds every kernel of libaesw_shplonk.so
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
# The plan at the extents the kernels are written for: 16 sets over 16 super-set points.  t takes every value 1 ... 8, every point
# index occurs, set 0 has t = 2 (so that u can sit on a point inside it and on one outside), set 15 has t = 8 over the upper
# indices (mask bits 8 ... 15 alone); m = 1 but for the wide set (t = 1, m = 257: y^j past one stride of the prepare kernel's loop)
# and one of t = 8, m = 3.
FULL_K = 10
WIDE_SET, WIDE_COLS = 1, 257
FULL_SETS = (((0, 1), 1), ((2,), WIDE_COLS), ((3, 4, 5), 1), ((0, 6, 7, 9), 1), ((1, 2, 8, 10, 11), 1), ((3, 5, 12, 13, 14, 15), 1), ((0, 2, 4, 6, 8, 10, 12), 1),
             ((0, 1, 2, 3, 4, 5, 6, 7), 3), ((15,), 1), ((7, 14), 1), ((1, 9, 13), 1), ((4, 8, 11, 12), 1), ((5, 6, 10, 14, 15), 1), ((0, 3, 7, 9, 11, 13), 1),
             ((1, 2, 3, 5, 8, 13, 14), 1), ((8, 9, 10, 11, 12, 13, 14, 15), 1))
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


def full_points(k, seed=0x66756c6c):
    """16 super-set points: 0, 1, omega_k, r - 1 and twelve seeded values"""
    pts = [0, 1, nm.omega(k), nm.R - 1] + nm.seeded_values(12, seed + k)
    assert len(set(pts)) == len(pts) == 16
    return pts


def plan(sets=SETS, n_points=8):
    """column ids count up through the sets"""
    out, first = [], 0
    for idx, m in sets:
        out.append((idx, list(range(first, first + m))))
        first += m
    return Plan(range(n_points), out)


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


@functools.lru_cache(maxsize=None)
def full_stage(k=FULL_K):
    """stage()'s tuple for FULL_SETS over full_points(k): seeded columns, their own evaluations"""
    p, pts = plan(FULL_SETS, 16), full_points(k)
    columns = [[nm.seeded_values(1 << k, 0x66630000 + 1024 * k + c) for c in cols] for _idx, cols in p.sets]
    evals = [[[om.evaluate(column, pts[q]) for q in idx] for column in columns[i]] for i, (idx, _cols) in enumerate(p.sets)]
    y, v, u = nm.seeded_values(3, 0x667976 + k)
    return p, pts, columns, evals, y, v, u


def with_challenges(stage, y=None, v=None, u=None):
    """the stage with other challenges"""
    return tuple(stage[:4]) + tuple(old if new is None else new for old, new in zip(stage[4:], (y, v, u)))


def u_on_a_point():
    """name -> the full stage with u on a super-set point: outside set 0 (z_0 = 0, and with it z_T) and inside it (z_T = 0 alone)"""
    stage = full_stage()
    p, pts = stage[0], stage[1]
    outside, inside = max(set(range(len(pts))) - set(p.sets[0][0])), p.sets[0][0][-1]
    return {"u_outside_set_0": with_challenges(stage, u=pts[outside]), "u_inside_set_0": with_challenges(stage, u=pts[inside])}


def degenerate_stages(k=10):
    """name -> stage(k) with y, v at 0 and 1, each at u = 0 (super-set point 0, which set 0 of SETS does not hold: z_0 = 0) and at
    the stage's own u"""
    stage_ = stage(k)
    out = {}
    for name, y, v in (("y=0", 0, None), ("v=0", None, 0), ("y=v=1", 1, 1)):
        out[name + ",u=0"] = with_challenges(stage_, y, v, 0)
        out[name] = with_challenges(stage_, y, v)
    return out


def flat_evals(evals):
    """d_evals: set by set, column by column, point by point"""
    return [e for of_set in evals for of_column in of_set for e in of_column]


def launched():
    return {"%s::shplonk_%s_kernel" % (NAMESPACE, name) for name in ("prepare", "finish", "powers", "chunk", "carry", "report")} | \
        {"%s::shplonk_%s_kernel<%d>" % (NAMESPACE, name, m) for name in ("combine", "scan") for m in STORE_MODES}
