"""aesw_theta_compress_table_device / Context.compress_table on the GPU: all 3 x 66 561 cells against tests/theta_model.py --
plain integers mod r over the byte columns of the lookup table -- for theta in {0, 1, r - 1, two seeded random values}, the
reference, the FIPS and one random non-xtime table set; a theta that is not canonical; a captured call that follows the 32
bytes of theta from replay to replay.  The tables and the report lie in poisoned, guard-banded buffers (tests/guarded.py)."""
import numpy as np
import pytest

import guarded as G
import oracle_lib
import theta_cases as tc
import theta_model as tm

pytestmark = pytest.mark.gpu
OK, INVALID = 0, 1


def thetas():
    out = [0, 1, tc.R - 1]
    for seed in tc.THETA_SEEDS:
        out.append(int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % tc.R)
    return out


@pytest.fixture(scope="module")
def worlds(pkg, ctx, oracle):
    """name -> (context, uint8[4, 66561] table bytes from the ORACLE's tables)"""
    made = {"reference": (ctx, oracle.lookup_table())}
    for name, t in (("fips", oracle.fips_tables()), ("random", G.random_tables())):
        made[name] = (pkg.Context(0, tables=t), oracle_lib.Oracle(tables=t).lookup_table())
    yield made
    for name in ("fips", "random"):
        made[name][0].close()


class Call:
    def __init__(self, pkg, ctx, arena):
        import torch
        self.torch, self.pkg, self.ctx, self.arena, self.lib = torch, pkg, ctx, arena, pkg.api.load_theta_library()
        self.out, self.rep = arena.out("table_fr", 3 * tm.BINS * 32, (3, tm.BINS, 32)), arena.out("report", 16)
        self.theta = torch.zeros(32, dtype=torch.uint8, device="cuda")

    def set_theta(self, raw: int):
        self.theta.copy_(self.torch.from_numpy(np.frombuffer(raw.to_bytes(32, "little"), np.uint8).copy()))

    def run(self, expect=OK, h=None, theta=0, out=0, rep=0):
        arg = lambda given, t: t.data_ptr() if given == 0 else given  # noqa: E731
        rc = self.lib.aesw_theta_compress_table_device(self.ctx._h if h is None else h, arg(theta, self.theta), arg(out, self.out), arg(rep, self.rep),
                                                       self.ctx._stream())
        assert rc == expect, (rc, self.ctx._lib.aesw_last_error(self.ctx._h))

    def result(self):
        self.torch.cuda.synchronize()
        self.arena.check()
        return self.out.cpu().numpy(), self.pkg.api.theta_report_dict(self.rep.view(self.torch.int64))


@pytest.mark.parametrize("which", ("reference", "fips", "random"))
def test_every_cell_is_the_models(pkg, worlds, which):
    ctx, table = worlds[which]
    for i, theta in enumerate(thetas()):
        c = Call(pkg, ctx, G.DeviceArena(G.CANARIES[i % 2]))
        c.set_theta(theta * (1 << 256) % tc.R)
        c.run()
        got, rep = c.result()
        G.assert_bytes("%s theta %#x" % (which, theta), got, tm.compressed_tables(table, theta))
        assert rep == {"cells": 3 * tm.BINS, "noncanonical": False} and not got[:, tm.ZERO_ROW].any()
    # the Python face: an int is put into Montgomery form on the host
    theta = thetas()[-1]
    got, rep = ctx.compress_table(theta)
    assert np.array_equal(got.cpu().numpy(), tm.compressed_tables(table, theta)) and not rep["noncanonical"]


@pytest.mark.parametrize("raw", tc.NONCANONICAL)
def test_a_theta_that_is_not_canonical_gives_zero_tables_and_says_so(pkg, worlds, raw):
    ctx, _table = worlds["reference"]
    for canary in G.CANARIES:
        c = Call(pkg, ctx, G.DeviceArena(canary))
        c.set_theta(raw)
        c.run()
        got, rep = c.result()
        assert not got.any() and rep == {"cells": 3 * tm.BINS, "noncanonical": True}


def test_a_captured_call_follows_theta_from_replay_to_replay(pkg, worlds):
    import torch
    ctx, table = worlds["fips"]
    arena = G.DeviceArena()
    c = Call(pkg, ctx, arena)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        c.run()
    torch.cuda.synchronize()
    assert arena.poisoned_on_device(c.out) and arena.poisoned_on_device(c.rep), "the captured call ran during capture"
    for theta in (thetas()[3], None, thetas()[4]):
        c.set_theta(tc.R + 1 if theta is None else theta * (1 << 256) % tc.R)
        graph.replay()
        got, rep = c.result()
        if theta is None:
            assert not got.any() and rep["noncanonical"]
        else:
            G.assert_bytes("replay", got, tm.compressed_tables(table, theta))
            assert not rep["noncanonical"]
        arena.repoison()


def test_refusals_leave_the_outputs_alone_and_say_why(pkg, worlds):
    ctx, _ = worlds["reference"]
    c = Call(pkg, ctx, G.DeviceArena())
    err = lambda h=ctx: h._lib.aesw_last_error(h._h).decode()  # noqa: E731
    for kw, word in ((dict(theta=None), "d_theta"), (dict(theta=c.theta.data_ptr() + 4), "d_theta"), (dict(out=None), "d_table_fr"),
                     (dict(out=c.out.data_ptr() + 8), "d_table_fr"), (dict(rep=None), "d_report"), (dict(rep=c.rep.data_ptr() + 4), "d_report")):
        c.run(expect=INVALID, **kw)
        assert "aesw_theta_compress_table_device" in err() and word in err(), kw
    group = pkg.Group([0])
    try:
        c.run(expect=INVALID, h=group._h)
        assert "aesw_theta_compress_table_device" in err(group)
        with pytest.raises(pkg.AeswError):
            group.compress_table(1)
    finally:
        group.close()
    c.torch.cuda.synchronize()
    c.arena.check()
    assert c.arena.poisoned_on_device(c.out) and c.arena.poisoned_on_device(c.rep)
    with pytest.raises(ValueError):
        ctx.compress_table(c.theta[:16])
