"""The calls of libaesw_blind.so on the GPU through the C ABI: every refusal -- k out of bounds, first_row at or past 2^k, no column,
a tail above what the commitment takes, a pointer absent or misaligned, d_commit over an input, a null and a group context -- after
which nothing ran and every output still holds its poison; one captured graph of blinding_tail, commit_columns over bytes and
commit_tail, replayed twice with the seed rewritten in device memory in between, each replay the model's for its seed; and
examples/aesw_blind.c, plain C with no Python in the process, against the model's commitment."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import blind_cases as bc
import blind_model as bm
import guarded as G
import msm_model as mm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_every_refusal_leaves_the_poison_whole(pkg, ctx):
    import torch
    api = pkg.api
    lib = api.load_blind_library()
    k, n_cols, tail = bc.K, 2, 6
    n, first_row = 1 << k, (1 << k) - 6
    max_tail = int(lib.aesw_blind_max_tail())
    arena = G.DeviceArena()
    cells = arena.out("cells", n_cols * 32 * n)
    compact = arena.out("tail", n_cols * 32 * (max_tail + 1))
    commit = arena.out("commitments", 64 * n_cols)
    seed = ctx.blinding_seed(bc.SEED)
    tail_in = torch.from_numpy(bm.tail_cells(bc.SEED, k, n_cols, n - max_tail - 1, 1)).cuda()  # room for the 65 rows of a refused call
    basis = torch.from_numpy(bc.basis_cells(k)).cuda()
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    S, Cl, T, Cm, Ti, B = seed.data_ptr(), cells.data_ptr(), compact.data_ptr(), commit.data_ptr(), tail_in.data_ptr(), basis.data_ptr()
    refusals = []
    for f, out, name in (("rows", Cl, "d_cells"), ("tail", T, "d_tail")):
        refusals += [(f, (9, n_cols, first_row, 1, 0, S, out), "k must"), (f, (29, n_cols, 0, 1, 0, S, out), "k must"), (f, (k, 0, first_row, 1, 0, S, out), "n_cols"),
                     (f, (k, 65536, first_row, 1, 0, S, out), "n_cols"), (f, (k, n_cols, n, 1, 0, S, out), "first_row"), (f, (k, n_cols, 1 << 40, 1, 0, S, out), "first_row"),
                     (f, (k, n_cols, first_row, 1, 0, None, out), "d_seed"), (f, (k, n_cols, first_row, 1, 0, S + 8, out), "d_seed"),
                     (f, (k, n_cols, first_row, 1, 0, S, None), name), (f, (k, n_cols, first_row, 1, 0, S, out + 8), name),
                     (f, (k, n_cols, first_row, 1, 0, out + 32, out), "overlap")]
    refusals += [("commit_tail", (9, n_cols, first_row, Ti, B, Cm), "k must"), ("commit_tail", (29, n_cols, 0, Ti, B, Cm), "k must"),
                 ("commit_tail", (k, 0, first_row, Ti, B, Cm), "n_cols"), ("commit_tail", (k, 65536, first_row, Ti, B, Cm), "n_cols"),
                 ("commit_tail", (k, n_cols, n, Ti, B, Cm), "first_row"), ("commit_tail", (k, n_cols, n - max_tail - 1, Ti, B, Cm), "at most 64"),
                 ("commit_tail", (k, n_cols, 0, Ti, B, Cm), "at most 64"),
                 ("commit_tail", (k, n_cols, first_row, None, B, Cm), "d_tail"), ("commit_tail", (k, n_cols, first_row, Ti + 8, B, Cm), "d_tail"),
                 ("commit_tail", (k, n_cols, first_row, Ti, None, Cm), "d_basis"), ("commit_tail", (k, n_cols, first_row, Ti, B + 4, Cm), "d_basis"),
                 ("commit_tail", (k, n_cols, first_row, Ti, B, None), "d_commit"), ("commit_tail", (k, n_cols, first_row, Ti, B, Cm + 8), "d_commit"),
                 ("commit_tail", (k, n_cols, first_row, Cm + 64, B, Cm), "overlap"), ("commit_tail", (k, n_cols, first_row, Ti, Cm - 64 * (n - 1), Cm), "overlap"),
                 ("commit_tail", (k, n_cols, first_row, Ti, B, B + 64 * 5), "overlap"), ("commit_tail", (k, n_cols, first_row, Ti, B, Ti + 32), "overlap")]
    for f, args, word in refusals:
        assert getattr(lib, "aesw_blind_%s_device" % f)(ctx._h, *args, s) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_blind_%s_device" % f) in err() and word in err(), (f, args, word, err())
    assert lib.aesw_blind_rows_device(None, k, n_cols, first_row, 1, 0, S, Cl, s) == api.ERR_INVALID_ARG
    assert lib.aesw_blind_tail_device(None, k, n_cols, first_row, 1, 0, S, T, s) == api.ERR_INVALID_ARG
    assert lib.aesw_blind_commit_tail_device(None, k, n_cols, first_row, Ti, B, Cm, s) == api.ERR_INVALID_ARG
    group = pkg.Group([0, 0])  # a group context is refused by every call
    try:
        for f, args in (("rows", (k, n_cols, first_row, 1, 0, S, Cl)), ("tail", (k, n_cols, first_row, 1, 0, S, T)), ("commit_tail", (k, n_cols, first_row, Ti, B, Cm))):
            assert getattr(lib, "aesw_blind_%s_device" % f)(group._h, *args, s) == api.ERR_INVALID_ARG, f
    finally:
        group.close()
    torch.cuda.synchronize()
    arena.check()
    assert all(arena.poisoned_on_device(t) for t in (cells, compact, commit))
    G.assert_bytes("the basis is left alone", basis.cpu().numpy(), bc.basis_cells(k))
    G.assert_bytes("the seed is left alone", seed.cpu().numpy(), np.frombuffer(bc.SEED, np.uint8))
    # the Python face says the same before it calls (a Group's refusal is held by tests/test_blind_library.py)
    with pytest.raises(pkg.AeswError):
        ctx.blinding_tail(9, 1, 0, seed, 1)
    with pytest.raises(pkg.AeswError):
        ctx.blinding_tail(k, 1, n, seed, 1)
    with pytest.raises(pkg.AeswError):
        ctx.commit_tail(tail_in, k, n - max_tail - 1, basis, commit.view(n_cols, 64))
    with pytest.raises(ValueError):
        ctx.blind_rows(cells.view(n_cols, n, 32), k, first_row, seed[:16], 1)
    with pytest.raises(ValueError):
        ctx.commit_tail(tail_in[:, :tail].contiguous(), k, first_row, basis, commit.view(n_cols, 64)[:1])
    assert all(arena.poisoned_on_device(t) for t in (cells, compact, commit))


def test_a_captured_chain_follows_the_seed_through_two_replays(pkg, ctx):
    import torch
    k, n_cols, tail = bc.K, 3, 6
    n, first_row = 1 << k, (1 << k) - 6
    lib = pkg.api.load_msm_library()
    poison = 0xA5
    rng = np.random.default_rng(0x67726170)
    body = rng.integers(0, 256, (n_cols, n), dtype=np.uint8)
    body[:, first_row:] = 0
    d_body, d_basis = torch.from_numpy(body).cuda(), torch.from_numpy(bc.basis_cells(k)).cuda()
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_tail, d_commit = full(n_cols, tail, 32), full(n_cols, 64)
    workspace = full(int(lib.aesw_msm_workspace_bytes(k, n_cols, 1, 0)))
    held = ctx.blinding_seed(bc.SEEDS["zeros"])  # the 32 bytes the graph reads when it runs
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one stream, one linear chain
        ctx.blinding_tail(k, n_cols, first_row, held, bc.DOMAIN, out=d_tail)
        ctx.commit_columns(d_body, d_basis, out=d_commit, _workspace=workspace)
        ctx.commit_tail(d_tail, k, first_row, d_basis, d_commit)
    torch.cuda.synchronize()
    assert all(bool((x == poison).all()) for x in (d_tail, d_commit)), "the captured calls ran during capture"
    logs = [sum(int(b) * (mm.E0 + i * mm.D) for i, b in enumerate(column)) % mm.R for column in body]
    seen = []
    try:
        for name in ("random", "ones"):
            seed = bc.SEEDS[name]
            held.copy_(torch.from_numpy(np.frombuffer(seed, np.uint8).copy()).cuda())
            d_tail.fill_(poison)
            d_commit.fill_(poison)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            G.assert_bytes("the tail under the seed of %s" % name, d_tail.cpu().numpy(), bm.tail_cells(seed, k, n_cols, first_row, bc.DOMAIN))
            tails = bm.tail_values(seed, k, n_cols, first_row, bc.DOMAIN)
            for j in range(n_cols):
                G.assert_bytes("column %d under the seed of %s" % (j, name), d_commit[j].cpu().numpy(), bc.expected_commit(logs[j], tails[j], first_row))
            seen.append(d_commit.cpu().numpy().copy())
        assert not np.array_equal(seen[0], seen[1])
    finally:  # every tensor the graph names outlives it
        torch.cuda.synchronize()
        del graph
        torch.cuda.synchronize()
    assert all(t is not None for t in (d_body, d_basis, d_tail, d_commit, workspace, held, side))


def test_the_plain_c_example_prints_the_models_commitment(pkg, ctx, tmp_path):
    exe = tmp_path / "aesw_blind"
    lib_dir = ROOT / "halo2-aes_amd"
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", "/opt/rocm/include",
                    str(ROOT / "examples" / "aesw_blind.c"), "-o", str(exe), "-L", str(lib_dir), "-laesw_blind", "-laesw_msm", "-laesw", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + str(lib_dir), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    k, tail, seed = 10, 6, bytes(range(32))
    first_row = (1 << k) - tail
    body = sum(i % 251 for i in range(first_row))  # every basis point is G: a commitment's logarithm is the sum of its scalars
    for domain in (1, bc.BIG_DOMAIN):
        out = subprocess.run([str(exe), str(domain)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout
        said = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
        values = bm.tail_values(seed, k, 1, first_row, domain)[0]
        assert said["domain"] == str(domain) and said["tail"] == bm.tail_cells(seed, k, 1, first_row, domain).tobytes().hex()
        assert said["bytes"] == mm.to_points([mm.mul(body, mm.GENERATOR)]).tobytes().hex()
        assert said["commitment"] == mm.to_points([mm.mul(body + sum(values), mm.GENERATOR)]).tobytes().hex()
