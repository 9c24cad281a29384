"""libaesw_msm.so on the GPU against tests/msm_model.py, every byte of every commitment, on poisoned, guard-banded buffers.

k = 10 and 11, 1 and 3 columns, cells and bytes, slices 0 (the rule's), 1, 2 and 3 (an uneven last slice); at k = 10 also 65 columns:
the second workgroup of the combine kernel, its guard on the column, and a bucket grid 65 deep.  The columns of
tests/msm_cases.py: seeded scalars, all 0 (the identity: 64 zero bytes), all 1, all r - 1 (bytes: all 255), all the same value
(every row in one bucket per window), one non-zero row first and one last.  The basis has known logarithms, so an expectation is
one scalar multiplication of the model.  A basis of one repeated point (a bucket adds P to P) and one alternating P, -P under
equal scalars (the sum passes through the identity and ends there).  msm_basis: a round trip of good points, a point off the curve
at a named index, a coordinate at or above q, the report's count and first index."""
import numpy as np
import pytest

import guarded as G
import msm_cases as mc
import msm_model as mm

pytestmark = pytest.mark.gpu


def put(arena, name, array):
    """a guarded, 16-byte aligned device copy of a uint8 array"""
    import torch
    t = arena.out(name, array.size, array.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(array)).to(t.device))
    return t


@pytest.fixture(scope="module")
def bases(ctx):
    """k -> the basis of known logarithms on the device, built once by the model"""
    import torch
    return {k: torch.from_numpy(mc.basis_cells(k)).cuda() for k in mc.KS}


def commit(pkg, ctx, arena, kind, k, scalars, basis, slices):
    n_cols = scalars.shape[0]
    ws = arena.out("ws", int(pkg.api.load_msm_library().aesw_msm_workspace_bytes(k, n_cols, kind, slices)))
    got = ctx.commit_columns(put(arena, "scalars", scalars), basis, out=arena.out("out", n_cols * 64, (n_cols, 64)), slices=slices, _workspace=ws)
    arena.check()
    return got.cpu().numpy()


@pytest.mark.parametrize("slices", mc.SLICES)
@pytest.mark.parametrize("n_cols", mc.COLS)
@pytest.mark.parametrize("kind", (mc.FR, mc.BYTES), ids=mc.kind_name)
@pytest.mark.parametrize("k", mc.KS)
def test_every_column_is_the_model(pkg, ctx, bases, k, kind, n_cols, slices):
    for i, names in enumerate(mc.groups(kind, k, n_cols)):
        scalars = np.stack([mc.scalar_bytes(kind, mc.columns(kind, k)[name]) for name in names])
        got = commit(pkg, ctx, G.DeviceArena(G.CANARIES[i % 2]), kind, k, scalars, bases[k], slices)
        for name, row in zip(names, got):
            G.assert_bytes("k=%d %s slices=%d column %s" % (k, mc.kind_name(kind), slices, name), row, mc.expected(kind, k, name))
    assert not mc.expected(kind, k, "zero").any()  # the identity is 64 zero bytes


MANY_COLS = 65  # the combine kernel takes 64 columns a workgroup: a second one, of which one lane works
WORKSPACE_LIMIT = 256 << 20


@pytest.mark.parametrize("kind,slices", ((mc.BYTES, 3), (mc.FR, 0)), ids=("bytes-3", "fr-0"))
def test_many_columns_reach_the_second_workgroup_of_the_combine(pkg, ctx, bases, kind, slices):
    k = mc.KS[0]
    need = int(pkg.api.load_msm_library().aesw_msm_workspace_bytes(k, MANY_COLS, kind, slices))
    if need > WORKSPACE_LIMIT:
        pytest.skip("the workspace of %d columns at k = %d is %d bytes, above %d" % (MANY_COLS, k, need, WORKSPACE_LIMIT))
    named, n = mc.columns(kind, k), 1 << k
    # the named columns first; from there on seeded ones, no two of them equal
    later = lambda j: mm.seeded_scalars(n, 0x6d616e79 + j) if kind == mc.FR else [int(v) for v in np.random.default_rng(0x6d616e79 + j).integers(0, 256, n)]  # noqa: E731
    cols = [named[sorted(named)[j % 7]] if j < 7 else later(j) for j in range(MANY_COLS)]
    assert len({tuple(c) for c in cols[7:]}) == MANY_COLS - 7 and len(named) == 7
    arena = G.DeviceArena(G.CANARIES[kind])
    got = commit(pkg, ctx, arena, kind, k, np.stack([mc.scalar_bytes(kind, c) for c in cols]), bases[k], slices)  # commit checks the guards: the one behind out is whole
    assert got.shape == (MANY_COLS, 64) and not (got[64] == arena.canary).all()  # out[64] is written
    for j, c in enumerate(cols):
        G.assert_bytes("k=%d %s slices=%d column %d of %d" % (k, mc.kind_name(kind), slices, j, MANY_COLS), got[j], mm.to_points([mm.known_commit(c)])[0])


@pytest.mark.parametrize("kind", (mc.FR, mc.BYTES), ids=mc.kind_name)
def test_a_repeated_point_and_an_alternating_basis(pkg, ctx, kind):
    import torch
    k = mc.KS[0]
    p = mm.known_basis(1)[0]
    cols = [mc.columns(kind, k)[name] for name in ("seeded", "same")]
    scalars = np.stack([mc.scalar_bytes(kind, c) for c in cols])
    repeated = torch.from_numpy(mm.to_points([p] * (1 << k))).cuda()
    got = commit(pkg, ctx, G.DeviceArena(), kind, k, scalars, repeated, 2)
    assert mm.from_points(got) == [mm.mul(sum(c), p) for c in cols]
    alternating = torch.from_numpy(mm.to_points([p, mm.neg(p)] * (1 << (k - 1)))).cuda()
    got = commit(pkg, ctx, G.DeviceArena(G.CANARIES[1]), kind, k, scalars, alternating, 3)
    assert mm.from_points(got) == [mm.mul(sum(cols[0][0::2]) - sum(cols[0][1::2]), p), None] and not got[1].any()
    assert pkg.api.g1_from_cells(got) == mm.from_points(got)


def test_cells_that_are_not_canonical_leave_the_guard_bands_whole(pkg, ctx, bases):
    k = mc.KS[1]
    got = commit(pkg, ctx, G.DeviceArena(), mc.FR, k, np.full((3, 1 << k, 32), 0xFF, np.uint8), bases[k], 3)
    assert got.shape == (3, 64) and not (got.reshape(-1, 8) == 0xA5).all(axis=1).any()  # every commitment was written


def test_the_basis_call_converts_checks_and_reports(pkg, ctx):
    import torch
    k = mc.KS[0]
    points = mm.known_basis(1 << k)
    canonical = mm.canonical_points(points)
    arena = G.DeviceArena()
    got = ctx.msm_basis(put(arena, "points", canonical), out=arena.out("basis", canonical.size, canonical.shape), _report=arena.out("report", 16))
    arena.check()
    G.assert_bytes("the basis", got.cpu().numpy(), mc.basis_cells(k))
    assert torch.equal(ctx.msm_basis(canonical), got)  # a numpy array is uploaded
    d_in = torch.from_numpy(canonical).cuda()
    assert ctx.msm_basis(d_in, out=d_in) is d_in and torch.equal(d_in, got)  # in place
    assert np.array_equal(pkg.api.g1_generator(), mm.to_points([mm.GENERATOR])[0])
    # a point off the curve at 700, a coordinate at or above q at 300 and at 1023: three bad points, the first at 300
    bad = canonical.copy()
    bad[700, 32] ^= 1
    bad[300, :32] = np.frombuffer((points[300][0] + mm.Q).to_bytes(32, "little"), np.uint8)
    bad[1023, 32:] = 0xFF
    lib = pkg.api.load_msm_library()
    arena = G.DeviceArena(G.CANARIES[1])
    report = arena.out("report", 16)
    assert lib.aesw_msm_basis_device(ctx._h, k, put(arena, "points", bad).data_ptr(), arena.out("basis", bad.size).data_ptr(), report.data_ptr(), ctx._stream()) == 0
    arena.check()
    assert [int(v) for v in report.cpu().numpy().view(np.uint64)] == [3, 300]
    with pytest.raises(pkg.AeswError, match="3 of the 2\\^10 points .* index 300"):
        ctx.msm_basis(bad)
    bad = canonical.copy()
    bad[5] = 0  # x = y = 0 is the identity's encoding, and no point of a basis
    with pytest.raises(pkg.AeswError, match="1 of the .* index 5"):
        ctx.msm_basis(bad)
