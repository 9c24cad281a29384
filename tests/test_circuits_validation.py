"""The host-side checks of the many-circuit Python calls (CPU): bad block counts raise before anything is launched.

Context's circuit methods validate `counts` first, so a Context whose C library records every call shows that nothing
reached the library when they raise."""
import numpy as np
import pytest


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _fake_ctx(pkg):
    ctx = object.__new__(pkg.Context)
    ctx._lib = _Recorder()
    ctx._h = None
    ctx.device = 0
    return ctx


def test_circuit_offsets(pkg):
    cap = pkg.block_capacity(14, 1)
    assert cap == 10
    offs = pkg.circuit_offsets(14, 1, [10, 0, 3], 13)
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 10, 10, 13]
    with pytest.raises(ValueError, match="holds 0 ... 10"):
        pkg.circuit_offsets(14, 1, [10, 11], 21)
    with pytest.raises(ValueError, match="sum to 12"):
        pkg.circuit_offsets(14, 1, [10, 2], 13)
    with pytest.raises(ValueError, match="at least one circuit"):
        pkg.circuit_offsets(14, 1, [], 0)
    with pytest.raises(ValueError):
        pkg.circuit_offsets(14, 1, [-1, 2], 1)


@pytest.mark.parametrize("counts,n,what", [([10, 11], 21, "holds"), ([4, 4], 9, "sum to"), ([], 0, "at least one")],
                         ids=["over-capacity", "wrong-sum", "no-circuits"])
def test_circuit_calls_raise_before_any_launch(pkg, counts, n, what):
    ctx = _fake_ctx(pkg)
    pt = np.zeros((n, 16), np.uint8)
    keys = np.zeros((max(len(counts), 1), 16), np.uint8)
    wit = pkg.Witness(*[np.zeros(n * pkg.column_stride(pkg.LAYOUT_PACKED, c), np.uint8) for c in range(3)], None, None)
    kw = pkg.KeyWitness(np.zeros(96 * len(keys), np.uint8), None, None, None, None)
    with pytest.raises(ValueError, match=what):
        ctx.assemble_advice_circuits(14, 1, wit, kw, counts, as_fr=True, n_blocks=n)
    with pytest.raises(ValueError, match=what):
        ctx.circuits(14, 1, keys, pt, counts)
    assert ctx._lib.calls == []


def test_group_refuses_the_circuit_calls(pkg):
    g = object.__new__(pkg.Group)
    for name in ("assemble_advice_circuits", "circuits"):
        with pytest.raises(pkg.AeswError):
            getattr(g, name)()
