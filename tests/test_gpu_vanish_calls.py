"""The calls of libaesw_vanish.so on the GPU one by one, through the C ABI: each segment alone from a seeded acc_in, in place and
out of place, against tests/vanish_model.py on every row; the whole fold -- tables, scalars, every segment, the division -- captured
as one linear chain on one side stream and replayed twice with the four challenges rewritten in device memory in between; and
every refusal, after which nothing ran and every output still holds its poison."""
import numpy as np
import pytest

import guarded as G
import ntt_model as nm
import vanish_cases as vc
import vanish_gpu as vg
import vanish_model as vm

pytestmark = pytest.mark.gpu
CASE = vc.FULL[0]


class World:
    """the seeded columns of CASE on the device, the tables, the scalars and a seeded acc_in, and the C calls over them"""

    def __init__(self, pkg, ctx, arena):
        import torch
        self.pkg, self.ctx, self.arena = pkg, ctx, arena
        self.lib = pkg.api.load_vanish_library()
        self.k, self.ext_k, self.zeta_sel, self.n_sets, self.chunk_len = CASE
        self.rows = 1 << self.ext_k
        self.cells, self.values = vg.columns(self.ext_k, self.n_sets, self.chunk_len)
        self.d = vg.upload(self.cells)
        self.perm_sets = pkg.api.permutation_sets(self.n_sets, self.chunk_len)
        self.set_values = [torch.from_numpy(vg.values_of_set(self.cells, self.n_sets, self.chunk_len, s)).cuda() for s in range(self.perm_sets)]
        self.tables = ctx.vanishing_tables(self.k, self.ext_k, self.zeta_sel)
        self.scalars = ctx.vanishing_scalars(self.n_sets, self.chunk_len, *vg.challenges())
        self.seeded = nm.seeded_values(self.rows, 0x61636369)
        self.shape = (self.k, self.ext_k, self.n_sets, self.chunk_len, vc.n_rows(self.k))

    def args(self, kind, s):
        """the pointers of a segment call between the shape and d_acc_in"""
        d, p = self.d, lambda t: t.data_ptr()  # noqa: E731
        if kind == "head":
            return (p(d["advice"][3 * self.n_sets]), p(d["rcon"]), p(d["zperm"]), p(d["l"]), p(self.scalars))
        if kind == "perm":
            first = s * self.chunk_len
            return (s, p(self.set_values[s]), p(d["sigma"][first:]), p(d["zperm"][s]), p(d["l"]), p(self.tables), p(self.scalars))
        five = 5 * s
        return (s, p(d["advice"][3 * s:]), p(d["selectors"][five:]), p(d["table"]), p(d["a"][five:]), p(d["s"][five:]), p(d["zlookup"][five:]), p(d["l"]), p(self.scalars))

    def call(self, kind, s, acc_in, acc_out):
        f = getattr(self.lib, "aesw_vanish_%s_device" % kind)
        if kind == "divide":
            rc = f(self.ctx._h, self.k, self.ext_k, self.tables.data_ptr(), acc_in.data_ptr(), acc_out.data_ptr(), self.ctx._stream())
        elif kind == "head":
            rc = f(self.ctx._h, *self.shape, *self.args(kind, s), acc_out.data_ptr(), self.ctx._stream())
        else:
            rc = f(self.ctx._h, *self.shape, *self.args(kind, s), acc_in.data_ptr(), acc_out.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, "aesw_vanish_%s_device" % kind)

    def model(self, kind, s, acc_in):
        sc = vm.scalars(self.n_sets, self.chunk_len, *vg.challenges())
        cell = lambda g, c, r: self.values[g][c][r]  # noqa: E731
        return nm.to_cells([vm.run_segment(kind, s, self.k, self.ext_k, self.zeta_sel, self.n_sets, self.chunk_len, vc.n_rows(self.k), j, cell, sc, acc_in[j])
                            for j in range(self.rows)])


def test_each_segment_alone_from_a_seeded_acc_in_place_and_out_of_place(pkg, ctx):
    arena = G.DeviceArena(G.CANARIES[1])
    w = World(pkg, ctx, arena)
    for kind, s in vm.segments(w.n_sets, w.chunk_len):
        want = w.model(kind, s, [0] * w.rows if kind == "head" else w.seeded)
        acc_in = vg.put(arena, "acc_in", nm.to_cells(w.seeded))
        out = arena.out("out", 32 * w.rows, (w.rows, 32))
        w.call(kind, s, acc_in, out)
        same = vg.put(arena, "same", nm.to_cells(w.seeded))
        w.call(kind, s, same, same)
        arena.check()
        G.assert_bytes("%s(%d) out of place" % (kind, s), out.cpu().numpy(), want)
        G.assert_bytes("%s(%d) in place" % (kind, s), same.cpu().numpy(), want)
        G.assert_bytes("%s(%d) leaves acc_in alone" % (kind, s), acc_in.cpu().numpy(), nm.to_cells(w.seeded))


def test_the_captured_fold_follows_the_challenges_through_two_replays(pkg, ctx):
    import torch
    k, ext_k, zeta_sel, n_sets, chunk_len = CASE
    lib = pkg.api.load_vanish_library()
    poison = 0xA5
    cells, _values = vg.columns(ext_k, n_sets, chunk_len)
    d = vg.upload(cells)
    seeds = (0x7663686c, 0x72657032)
    full = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device="cuda")  # noqa: E731
    tables, scalars, acc_cells = full(int(lib.aesw_vanish_tables_bytes(k, ext_k))), full(int(lib.aesw_vanish_scalars_bytes(n_sets, chunk_len))), full(1 << ext_k, 32)
    held = torch.from_numpy(nm.to_cells(list(vg.challenges(seeds[0])))).cuda()  # theta, beta, gamma, y: four cells the graph reads when it runs
    values = [torch.from_numpy(vg.values_of_set(cells, n_sets, chunk_len, s)).cuda() for s in range(pkg.api.permutation_sets(n_sets, chunk_len))]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one stream, one linear chain
        ctx.vanishing_tables(k, ext_k, zeta_sel, _out=tables)
        ctx.vanishing_scalars(n_sets, chunk_len, held[0], held[1], held[2], held[3], _out=scalars)
        acc = ctx.quotient_accumulator(k, ext_k, zeta_sel, n_sets, chunk_len, vc.n_rows(k), tables, scalars, _acc=acc_cells)
        out = vg.fold(ctx, acc, d, values, n_sets)
    torch.cuda.synchronize()
    assert out.data_ptr() == acc_cells.data_ptr()
    assert all(bool((x == poison).all()) for x in (tables, scalars, acc_cells)), "the captured calls ran during capture"
    try:
        for seed in seeds:
            held.copy_(torch.from_numpy(nm.to_cells(list(vg.challenges(seed)))).cuda())
            acc_cells.fill_(poison)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            G.assert_bytes("the replay under the challenges of seed %#x" % seed, acc_cells.cpu().numpy(), vg.expected(CASE, seed))
        assert not np.array_equal(vg.expected(CASE, seeds[0]), vg.expected(CASE, seeds[1]))
    finally:  # every tensor the graph names outlives it
        torch.cuda.synchronize()
        del graph
        torch.cuda.synchronize()
    assert all(t is not None for t in (tables, scalars, acc_cells, held, values, d, side))


def test_every_refusal_leaves_the_poison_whole(pkg, ctx):
    import torch
    api = pkg.api
    arena = G.DeviceArena()
    w = World(pkg, ctx, arena)
    lib, k, e, N, L, U = w.lib, w.k, w.ext_k, w.n_sets, w.chunk_len, vc.n_rows(w.k)
    out = arena.out("out", 2 * 32 * w.rows)
    tables, scalars = arena.out("tables", int(lib.aesw_vanish_tables_bytes(k, e))), arena.out("scalars", int(lib.aesw_vanish_scalars_bytes(N, L)))
    acc_in = torch.from_numpy(nm.to_cells(w.seeded)).cuda()
    ch = torch.from_numpy(nm.to_cells(list(vg.challenges()))).cuda()
    err = lambda: ctx._lib.aesw_last_error(ctx._h).decode()  # noqa: E731
    s = ctx._stream()
    o, a, T, S_, c = out.data_ptr(), acc_in.data_ptr(), w.tables.data_ptr(), w.scalars.data_ptr(), ch.data_ptr()
    head, perm, look = w.args("head", 0), w.args("perm", 0)[1:], w.args("lookup", 0)[1:]
    swap = lambda args, i, v: args[:i] + (v,) + args[i + 1:]  # noqa: E731
    shape = (k, e, N, L, U)
    shapes = [((9, e, N, L, U), "k must"), ((k, 11, N, L, U), "k must"), ((k, 29, N, L, U), "k must"), ((k, e, 0, L, U), "n_sets"), ((k, e, 1025, L, U), "n_sets"),
              ((k, e, N, 0, U), "chunk_len"), ((k, e, N, 4, U), "chunk_len"), ((k, e, N, L, 0), "n_rows"), ((k, e, N, L, 1 << k), "n_rows")]
    refusals = []
    for bad, word in shapes:  # the bounds are those of every segment call
        refusals += [("head", bad + head + (o,), word), ("perm", bad + (0,) + perm + (a, o), word), ("lookup", bad + (0,) + look + (a, o), word)]
    refusals += [("perm", shape + (w.perm_sets,) + perm + (a, o), "set"), ("lookup", shape + (N,) + look + (a, o), "set")]
    names = {"head": ("d_words", "d_rcon", "d_zperm", "d_l", "d_scalars"), "perm": ("d_values", "d_sigma", "d_z", "d_l", "d_tables", "d_scalars"),
             "lookup": ("d_advice3", "d_selectors5", "d_table4", "d_a5", "d_s5", "d_z5", "d_l", "d_scalars")}
    for kind, args in (("head", head), ("perm", perm), ("lookup", look)):
        tail = (o,) if kind == "head" else (a, o)
        front = shape if kind == "head" else shape + (0,)
        for i, name in enumerate(names[kind]):  # every pointer: absent, misaligned, and overlapped by the output
            refusals += [(kind, front + swap(args, i, None) + tail, name), (kind, front + swap(args, i, args[i] + 8) + tail, name),
                         (kind, front + swap(args, i, o + 64) + tail, "overlap")]
        refusals += [(kind, front + args + tail[:-1] + (None,), "d_acc_out"), (kind, front + args + tail[:-1] + (o + 4,), "d_acc_out")]
        if kind != "head":
            refusals += [(kind, front + args + (None, o), "d_acc_in"), (kind, front + args + (a + 8, o), "d_acc_in"), (kind, front + args + (o + 32, o), "d_acc_in")]
    refusals += [("divide", (9, e, T, a, o), "k must"), ("divide", (k, 11, T, a, o), "k must"), ("divide", (k, e, None, a, o), "d_tables"), ("divide", (k, e, T + 8, a, o), "d_tables"),
                 ("divide", (k, e, T, None, o), "d_acc_in"), ("divide", (k, e, T, a + 4, o), "d_acc_in"), ("divide", (k, e, T, a, None), "d_acc_out"),
                 ("divide", (k, e, T, a, o + 8), "d_acc_out"), ("divide", (k, e, T, o + 32, o), "d_acc_in"), ("divide", (k, e, o + 64, a, o), "overlap"),
                 ("tables", (9, e, 1, tables.data_ptr()), "k must"), ("tables", (k, 11, 1, tables.data_ptr()), "k must"), ("tables", (k, e, 2, tables.data_ptr()), "zeta_sel"),
                 ("tables", (k, e, 1, None), "d_tables"), ("tables", (k, e, 1, tables.data_ptr() + 8), "d_tables"),
                 ("scalars", (0, L, c, c + 32, c + 64, c + 96, scalars.data_ptr()), "n_sets"), ("scalars", (N, 9, c, c + 32, c + 64, c + 96, scalars.data_ptr()), "chunk_len"),
                 ("scalars", (N, L, None, c + 32, c + 64, c + 96, scalars.data_ptr()), "d_theta"), ("scalars", (N, L, c, c + 40, c + 64, c + 96, scalars.data_ptr()), "d_beta"),
                 ("scalars", (N, L, c, c + 32, None, c + 96, scalars.data_ptr()), "d_gamma"), ("scalars", (N, L, c, c + 32, c + 64, c + 100, scalars.data_ptr()), "d_y"),
                 ("scalars", (N, L, c, c + 32, c + 64, c + 96, None), "d_scalars"), ("scalars", (N, L, c, c + 32, c + 64, c + 96, scalars.data_ptr() + 8), "d_scalars"),
                 ("scalars", (N, L, c, c + 32, c + 64, scalars.data_ptr() + 64, scalars.data_ptr()), "overlap")]
    for f, args, word in refusals:
        assert getattr(lib, "aesw_vanish_%s_device" % f)(ctx._h, *args, s) == api.ERR_INVALID_ARG, (f, args)
        assert ("aesw_vanish_%s_device" % f) in err() and word in err(), (f, args, word, err())
    assert lib.aesw_vanish_tables_device(None, k, e, 1, tables.data_ptr(), s) == api.ERR_INVALID_ARG
    assert lib.aesw_vanish_scalars_device(None, N, L, c, c + 32, c + 64, c + 96, scalars.data_ptr(), s) == api.ERR_INVALID_ARG
    assert lib.aesw_vanish_head_device(None, *shape, *head, o, s) == api.ERR_INVALID_ARG
    assert lib.aesw_vanish_perm_device(None, *shape, 0, *perm, a, o, s) == api.ERR_INVALID_ARG
    assert lib.aesw_vanish_lookup_device(None, *shape, 0, *look, a, o, s) == api.ERR_INVALID_ARG
    assert lib.aesw_vanish_divide_device(None, k, e, T, a, o, s) == api.ERR_INVALID_ARG
    torch.cuda.synchronize()
    arena.check()
    assert all(arena.poisoned_on_device(t) for t in (out, tables, scalars))
    G.assert_bytes("acc_in is left alone", acc_in.cpu().numpy(), nm.to_cells(w.seeded))
    # the Python face says the same before it calls (a Group's refusal is held by tests/test_vanish_library.py)
    with pytest.raises(pkg.AeswError):
        ctx.vanishing_tables(9, 12)
    with pytest.raises(pkg.AeswError):
        ctx.vanishing_scalars(0, 3, 1, 2, 3, 4)
    with pytest.raises(ValueError):
        ctx.quotient_accumulator(k, e, 1, N, L, U, w.tables[:64], w.scalars)
