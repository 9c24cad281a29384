"""The accumulator's cut rule (tests/acc_model.py) on the CPU: a run is covered exactly once by chunks that never cross a set
boundary, for every K in 9 ... 20 with 1 ... 4 sets, and summing tests/mult_model.py's contributions over any such cut gives
its histogram of the whole circuit -- "cutting does not matter", pinned against the oracle-held model, not against the kernel."""
import numpy as np
import pytest

import acc_cases as ac
import acc_model as am
import mult_model as mm

K, N = 14, 3


@pytest.mark.parametrize("k", range(9, 21))
def test_a_cut_covers_every_block_once_and_stays_inside_a_set(pkg, k):
    rng = np.random.default_rng(k)
    for n_sets in (1, 2, 3, 4):
        firsts = am.set_firsts(pkg.block_capacity, k, n_sets)
        cap = firsts[-1]
        assert cap == pkg.block_capacity(k, n_sets) and firsts == sorted(firsts)
        assert am.cut(firsts, 0, 0, 3) == [] and am.cut(firsts, cap, 0, 1) == []
        if cap == 0:
            continue
        runs = [(0, cap), (cap - 1, 1), (0, 1)] + [(int(a), int(rng.integers(0, cap - a + 1))) for a in rng.integers(0, cap, 6)]
        for first, n in runs:
            for chunk in (1, 2, 5, 7, 256, cap + 1):
                pieces = am.cut(firsts, first, n, chunk)
                covered = np.concatenate([np.arange(b, b + c) for _s, b, c in pieces] or [np.zeros(0, np.int64)])
                assert covered.tolist() == list(range(first, first + n)), (k, n_sets, first, n, chunk)
                for s, b, c in pieces:
                    assert 1 <= c <= chunk and firsts[s] <= b and b + c <= firsts[s + 1]
                    for j in (b, b + c - 1):  # the product's own placement agrees on the set and on the block's first row
                        assert tuple(pkg.block_placement(k, n_sets, j)) == (s, am.rows_of(firsts, s, j, 1).start), (k, n_sets, j)
                # at most one short chunk per set the run touches
                assert sum(1 for _s, _b, c in pieces if c < chunk) <= len({s for s, _b, _c in pieces})


@pytest.fixture(scope="module")
def circuit(oracle):
    rng = np.random.default_rng(0x616363)
    n = 31  # K = 14, N = 3 holds 10 + 12 + 12: the last set is partly filled
    with oracle.circuit(K, N, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8), record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * N + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * N + 1)])
    return n, adv, sel, oracle.tables()


@pytest.mark.parametrize("chunk", (1, 2, 5, 256))
def test_the_contributions_of_any_cut_sum_to_the_whole_circuit(pkg, circuit, chunk):
    n, adv, sel, tables = circuit
    whole, misses = mm.multiplicities(adv, sel, tables)
    assert misses == 0 and int(whole.sum()) == 400 + 1056 * n
    firsts = am.set_firsts(pkg.block_capacity, K, N)
    assert firsts == [0, 10, 22, 34]
    total, _ = am.key_contribution(mm, adv, sel, tables)
    assert int(total.sum()) == 400 and not total[1:].any()
    runs = ac.ragged(n)
    assert runs == [(0, 1), (1, 7), (8, 16), (24, 7)]
    for first, count in reversed(runs):
        for piece in am.cut(firsts, first, count, chunk):
            part, m = am.chunk_contribution(mm, adv, sel, tables, firsts, piece)
            assert m == 0 and int(part.sum()) == 1056 * piece[2] and int(part[piece[0]].sum()) == 1056 * piece[2]
            total += part
    assert np.array_equal(total, whole)
