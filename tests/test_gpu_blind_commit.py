"""The tail commitment of libaesw_blind.so on the GPU, over tests/msm_model.py's basis of known logarithms, so that an expectation is
one scalar multiplication: Context.commit_tail for tails of 1, 6, 63 and 64 rows with 1 and 3 columns, the tail cells led by
tests/field_cases.py's 0, 1, r - 1, the Montgomery 1 and a lone top limb, an incoming commitment that is the identity, a tail that
cancels the commitment exactly, a basis point that is the identity, two tail rows over equal basis points -- and the consistency
that is the point of the call: commit_blinded_bytes(bytes, tail) is, byte for byte, commit_columns over the same columns as Fr cells
with blind_rows applied, at k = 10 and at the smallest k at which a slice of the bucket method reaches a second chunk.  The
commitments lie in a poisoned, guard-banded buffer; every comparison is exact."""
import numpy as np
import pytest

import blind_cases as bc
import blind_model as bm
import guarded as G
import msm_cases as mc
import msm_model as mm

pytestmark = pytest.mark.gpu
LOGS = (0x636f6d6d6974, 0, 0x31)  # the incoming commitments, as logarithms: column 1 comes in as the identity


def run(ctx, arena, k, first_row, tails, commits, basis_cells):
    """commit_tail of plain tails [n_cols][tail] onto the points `commits`, which lie guarded; returns the points after"""
    import torch
    n_cols, tail = len(tails), len(tails[0])
    d_tail = torch.from_numpy(mm.scalar_cells([v for column in tails for v in column]).reshape(n_cols, tail, 32)).cuda()
    d_basis = torch.from_numpy(basis_cells).cuda()
    d_commit = arena.out("commitments", 64 * n_cols, (n_cols, 64))
    d_commit.copy_(torch.from_numpy(mm.to_points(commits)).cuda())
    assert ctx.commit_tail(d_tail, k, first_row, d_basis, d_commit) is d_commit
    arena.check()
    G.assert_bytes("the tail is left alone", d_tail.cpu().numpy(), mm.scalar_cells([v for column in tails for v in column]).reshape(n_cols, tail, 32))
    return d_commit.cpu().numpy()


@pytest.mark.parametrize("n_cols", bc.COLS)
@pytest.mark.parametrize("tail", bc.COMMIT_TAILS)
def test_the_tail_is_added_to_the_commitment(pkg, ctx, n_cols, tail):
    k = bc.K
    first_row = (1 << k) - tail
    assert tail <= int(pkg.api.load_blind_library().aesw_blind_max_tail())
    tails = bc.commit_tail_values(tail, n_cols)
    commits = [mm.mul(LOGS[j], mm.GENERATOR) for j in range(n_cols)]
    got = run(ctx, G.DeviceArena(G.CANARIES[tail % 2]), k, first_row, tails, commits, bc.basis_cells(k))
    for j in range(n_cols):
        G.assert_bytes("column %d of %d, %d rows" % (j, n_cols, tail), got[j], bc.expected_commit(LOGS[j], tails[j], first_row))


def test_the_special_cells_one_by_one_onto_the_identity(pkg, ctx):
    k, specials = bc.K, bc.special_cells()
    first_row = (1 << k) - 1  # a tail of one row: the term alone
    import torch
    d_basis = torch.from_numpy(bc.basis_cells(k)).cuda()
    arena = G.DeviceArena()
    d_commit = arena.out("commitments", 64 * len(specials), (len(specials), 64))
    d_commit.zero_()
    d_tail = torch.from_numpy(bc.raw_cells(specials).reshape(len(specials), 1, 32)).cuda()
    ctx.commit_tail(d_tail, k, first_row, d_basis, d_commit)
    arena.check()
    got = d_commit.cpu().numpy()
    for j, plain in enumerate(bm.plain_of_cells(bc.raw_cells(specials))):
        G.assert_bytes("the cell %#x" % specials[j], got[j], bc.expected_commit(0, [plain], first_row))
    assert not got[0].any() and got[1].any()  # zero times a point is the identity: 64 zero bytes


def test_a_tail_that_cancels_an_identity_in_the_basis_and_equal_points(pkg, ctx):
    k, tail = bc.K, 6
    n, first_row = 1 << k, (1 << k) - 6
    cancel = bc.cancelling_tail(LOGS[0], first_row, tail)
    got = run(ctx, G.DeviceArena(), k, first_row, [cancel], [mm.mul(LOGS[0], mm.GENERATOR)], bc.basis_cells(k))
    assert not got.any(), "commitment + tail = the identity: 64 zero bytes"
    basis = list(mm.known_basis(n))
    basis[first_row + 2] = None
    basis[first_row + 4] = basis[first_row + 3]
    values = bc.commit_tail_values(tail, 1)[0]
    got = run(ctx, G.DeviceArena(G.CANARIES[1]), k, first_row, [values], [None], mm.to_points(basis))
    G.assert_bytes("an identity and two equal points in the basis", got[0], mm.to_points([bm.commit_tail(None, values, basis[first_row:])])[0])
    # the same scalar on the two equal points, from a commitment that is that point too: P + P inside the law
    same = [5, 0, 0, 1, 1, 0]
    got = run(ctx, G.DeviceArena(), k, first_row, [same], [basis[first_row + 3]], mm.to_points(basis))
    G.assert_bytes("the commitment equal to a term", got[0], mm.to_points([bm.commit_tail(basis[first_row + 3], same, basis[first_row:])])[0])


def second_chunk_k(pkg, n_cols):
    """the smallest k at which a slice of commit_columns holds more rows than a chunk, for bytes and for cells"""
    lib = pkg.api.load_msm_library()
    chunk = int(lib.aesw_msm_chunk_rows())
    for k in range(10, 29):
        if all(-(-(1 << k) // int(lib.aesw_msm_slices(k, n_cols, kind, 0))) > chunk for kind in (mc.FR, mc.BYTES)):
            return k
    raise AssertionError("no k reaches a second chunk")


@pytest.mark.parametrize("which", ("k10", "second chunk"))
def test_the_blinded_byte_commitment_is_the_commitment_of_the_blinded_cells(pkg, ctx, which):
    import torch
    n_cols, tail = 2, 6
    k = bc.K if which == "k10" else second_chunk_k(pkg, n_cols)
    assert k == bc.K or k > bc.K
    n, first_row = 1 << k, (1 << k) - tail
    rng = np.random.default_rng(0x6279746573 + k)
    body = rng.integers(0, 256, (n_cols, n), dtype=np.uint8)
    body[:, first_row:] = 0  # the tail rows of the byte column are the tail's
    body[0, 0], body[1, first_row - 1] = 255, 255
    d_basis = torch.from_numpy(bc.basis_cells(k)).cuda()
    seed = ctx.blinding_seed(bc.SEED)
    # the cheap way: one 8-bit window over the bytes, then the tail's terms
    arena = G.DeviceArena()
    out = arena.out("commitments", 64 * n_cols, (n_cols, 64))
    d_tail = ctx.blinding_tail(k, n_cols, first_row, seed, bc.DOMAIN, bc.FIRST_COLUMN)
    assert ctx.commit_blinded_bytes(torch.from_numpy(body).cuda(), d_tail, k, first_row, d_basis, out=out) is out
    arena.check()
    # the dear way: the same columns as cells, blinded in place, all 32 windows
    mont = np.frombuffer(b"".join(bm.cell_bytes(v) for v in range(256)), np.uint8).reshape(256, 32)
    cells = torch.from_numpy(mont[body]).cuda()
    ctx.blind_rows(cells, k, first_row, seed, bc.DOMAIN, bc.FIRST_COLUMN)
    want = ctx.commit_columns(cells, d_basis)
    G.assert_bytes("commit_blinded_bytes against commit_columns over blinded cells, k = %d" % k, out.cpu().numpy(), want.cpu().numpy())
    # and both are the model's: the bytes' logarithm plus the tail's
    tails = bm.tail_values(bc.SEED, k, n_cols, first_row, bc.DOMAIN, bc.FIRST_COLUMN)
    for j in range(n_cols):
        log = sum(int(b) * (mm.E0 + i * mm.D) for i, b in enumerate(body[j])) % mm.R
        G.assert_bytes("column %d against the model" % j, out[j].cpu().numpy(), bc.expected_commit(log, tails[j], first_row))
