"""What the sweep of tests/test_gpu_ntt_transform.py cannot reach, with inputs whose transform is closed form.

A model run follows a column up to k = 18; NTT_PASS_LOG = 10 puts two full passes at k = 20 and the first three-pass plan at
k = 21 (nc.THREE_PASSES).  So here a column of three non-zero coefficients c_j at exponents e_j, one of them 2^k - 1, goes through
coeff_to_lagrange, and its evaluations sum c_j omega^(i e_j) are checked by pow at the first row, the last row, the first and last
cell of every pass boundary and 4 096 seeded rows; a dense seeded column goes through a round trip on the device.  Shapes: k = 21
(three passes; its middle pass is in place in the output), and nc.BIG, k = 22 with 33 columns, whose buffers pass 4 GiB each, with
the sparse column last: offsets are 64 bits.  k = 20 (two full passes exactly) and the plan of k = 28 are held on the CPU driver
only (tests/test_ntt_model.py): NO GPU CASE RUNS k > 22."""
import numpy as np
import pytest

import guarded as G
import ntt_cases as nc
import ntt_model as nm

pytestmark = pytest.mark.gpu


def sparse(k, seed):
    n = 1 << k
    rng = np.random.default_rng(seed)
    exps = (n - 1, int(rng.integers(1, n - 1)), int(rng.integers(1, n - 1)))
    return exps, nm.seeded_values(3, seed + 1)


def probe_rows(k, seed):
    n, P = 1 << k, nc.PASS_LOG
    edges = {0, n - 1}
    for s in range(P, k, P):  # the first and the last cell of every pass boundary
        edges |= {(1 << s) - 1, 1 << s, n - (1 << s), n - (1 << s) - 1}
    return sorted(edges | {int(v) for v in np.random.default_rng(seed).integers(0, n, 4096)})


def held(k, exps, coeffs, rows, cells):
    w = nm.omega(k)
    got = nm.from_cells(cells)
    for i, g in zip(rows, got):
        assert g == sum(c * pow(w, i * e, nm.R) for e, c in zip(exps, coeffs)) % nm.R, (k, i)


def test_three_passes_by_three_coefficients_and_a_dense_round_trip(ctx):
    import torch
    k = nc.THREE_PASSES
    tables = ctx.ntt_tables(k)
    exps, coeffs = sparse(k, 0x7233)
    arena = G.DeviceArena()
    col = arena.out("in", 2 * (32 << k), (2, 1 << k, 32))
    col.zero_()
    col[0, list(exps)] = torch.from_numpy(nm.to_cells(coeffs)).to(col.device)
    # the second column is dense: seeded bytes with the top byte cleared are canonical cells
    dense = torch.from_numpy(np.random.default_rng(0x7234).integers(0, 256, (1 << k, 32), dtype=np.uint8)).to(col.device)
    dense[:, 31] &= 0x1F
    col[1] = dense
    out = ctx.coeff_to_lagrange(col, k, tables, out=arena.out("out", 2 * (32 << k), (2, 1 << k, 32)))
    arena.check_on_device()
    rows = probe_rows(k, 0x7235)
    held(k, exps, coeffs, rows, out[0][rows].cpu().numpy())
    back = ctx.lagrange_to_coeff(out, k, tables, out=out)  # in place: through the workspace
    arena.check_on_device()
    assert torch.equal(back, col)


def test_buffers_beyond_four_gib_are_addressed_with_64_bit_offsets(ctx):
    import torch
    k, n_cols = nc.BIG
    nbytes = n_cols * (32 << k)
    assert nbytes > 1 << 32
    free, _total = torch.cuda.mem_get_info()
    if free < 2 * nbytes + (1 << 30):
        pytest.skip("the lease cannot allocate the %.1f GiB of input and output" % (2 * nbytes / 2 ** 30))
    tables = ctx.ntt_tables(k)
    exps, coeffs = sparse(k, 0x7242)
    arena = G.DeviceArena(G.CANARIES[1])
    col = arena.out("in", nbytes, (n_cols, 1 << k, 32))
    col.zero_()
    col[n_cols - 1, list(exps)] = torch.from_numpy(nm.to_cells(coeffs)).to(col.device)
    col[0, 1] = col[n_cols - 1, exps[0]]  # the first column is c x: a column that wrapped to offset 0 would show
    out = ctx.coeff_to_lagrange(col, k, tables, out=arena.out("out", nbytes, (n_cols, 1 << k, 32)))
    arena.check_on_device()
    rows = probe_rows(k, 0x7243)
    held(k, exps, coeffs, rows, out[n_cols - 1][rows].cpu().numpy())
    held(k, (1,), coeffs[:1], rows[:64], out[0][rows[:64]].cpu().numpy())
    assert not out[1:n_cols - 1].any()  # the columns between are zero and stay zero
    back = ctx.lagrange_to_coeff(out[n_cols - 1], k, tables)
    assert torch.equal(back, col[n_cols - 1])


def test_the_extended_transforms_over_three_passes_by_three_coefficients(ctx):
    """coeff_to_extended at ext_k = 21 from k = 19: row i is sum c_j zeta^(e_j mod 3) omega_ext^(i e_j) -- the zero padding and the zeta
    cycle in the bit-reversed first load of a three-pass plan --, and extended_to_coeff brings the coefficients back followed by
    zeros, out of place and in place: the zeta scale in the last store."""
    import torch
    ext_k, k, sel = nc.THREE_PASSES, nc.THREE_PASSES - 2, 1
    tables = ctx.ntt_tables(ext_k)
    exps, coeffs = sparse(k, 0x7245)
    arena = G.DeviceArena()
    col = arena.out("coeff", 2 * (32 << k), (2, 1 << k, 32))
    col.zero_()
    col[0, list(exps)] = torch.from_numpy(nm.to_cells(coeffs)).to(col.device)
    dense = torch.from_numpy(np.random.default_rng(0x7246).integers(0, 256, (1 << k, 32), dtype=np.uint8)).to(col.device)
    dense[:, 31] &= 0x1F
    col[1] = dense
    ext = ctx.coeff_to_extended(col, k, ext_k, tables, zeta_sel=sel, out=arena.out("ext", 2 * (32 << ext_k), (2, 1 << ext_k, 32)))
    arena.check_on_device()
    rows = probe_rows(ext_k, 0x7247)
    w, z = nm.omega(ext_k), nm.ZETAS[sel]
    got = nm.from_cells(ext[0][rows].cpu().numpy())
    for i, g in zip(rows, got):
        assert g == sum(c * pow(z, e % 3, nm.R) * pow(w, i * e, nm.R) for e, c in zip(exps, coeffs)) % nm.R, i
    back = ctx.extended_to_coeff(ext, ext_k, tables, zeta_sel=sel, out=arena.out("back", 2 * (32 << ext_k), (2, 1 << ext_k, 32)))
    arena.check_on_device()
    assert torch.equal(back[:, :1 << k], col) and not back[:, 1 << k:].any()
    again = ctx.extended_to_coeff(ext, ext_k, tables, zeta_sel=sel, out=ext)
    arena.check_on_device()
    assert torch.equal(again, back)
