"""tests/mult_model.py against the oracle's restated synthesize() (K = 15, N = 3): the model reads assembled byte columns and
selector columns only, so the oracle's circuit is its input as it stands."""
import numpy as np
import pytest

import mult_model as mm

K, N = 15, 3


@pytest.fixture(scope="module")
def circuit(oracle):
    rng = np.random.default_rng(0x6D756C74)
    cap = ((1 << K) - 1760) // 1360 + (N - 1) * ((1 << K) // 1360)
    n = cap - 5  # the last set is partly filled
    with oracle.circuit(K, N, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8), record_copies=False) as c:
        assert c.status == 0 and c.num_advice == 3 * N + 1 and c.num_selectors == 5 * N + 1
        adv = np.stack([c.advice(i) for i in range(3 * N + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * N + 1)])
    return n, adv, sel, oracle.tables()


def test_section_sums_are_the_selector_popcounts(circuit):
    n, adv, sel, tables = circuit
    hist, misses = mm.multiplicities(adv, sel, tables)
    assert misses == 0
    sums = mm.section_sums(hist)
    for s in range(N):
        for i in range(5):
            assert sums[s, i] == int(sel[5 * s + i].sum()), (s, i)
    assert not hist[:, 66560].any()
    # A block has 1 056 enabled lookups (608 Xor, 160 Sbox, 144 GfMul2, 144 GfMul3): 304 of its 1 360 rows -- the plaintext rows
    # and the MixColumns factors of 1 -- are plain copies.  The key schedule has 400.
    assert int(hist.sum()) == 400 + 1056 * n
    assert sums[:, 0].tolist() == [160, 0, 0]  # the range lookups are the key schedule's, in set 0


@pytest.mark.parametrize("tables", ("reference", "fips"))
def test_the_blocks_and_the_key_rows_add_up_to_the_circuit(oracle, tables):
    """block_histograms and key_histogram -- the yardstick of the GPU suites wherever a test itself says which blocks are counted --
    against the whole-circuit count of the oracle's K = 14 / N = 3 circuit with 31 blocks (10 + 12 + 9), placed by the oracle."""
    import oracle_lib
    k, n_sets, n = 14, 3, 31
    orc = oracle if tables == "reference" else oracle_lib.Oracle(tables=oracle.fips_tables())
    rng = np.random.default_rng(0x626C6B)
    with orc.circuit(k, n_sets, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8), record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
        sel = np.stack([c.selector(i) for i in range(5 * n_sets + 1)])
        places = [c.block_placement(b) for b in range(n)]
    assert [s for s, _row in places] == [0] * 10 + [1] * 12 + [2] * 9
    whole, misses = mm.multiplicities(adv, sel, orc.tables())
    assert misses == 0
    hist, block_misses = mm.block_histograms(adv, sel, orc.tables(), places)
    key, key_misses = mm.key_histogram(adv, sel, orc.tables())
    assert hist.shape == (n, mm.BINS) and not block_misses.any() and key_misses == 0
    assert hist.sum(axis=1).tolist() == [1056] * n and int(key.sum()) == 400
    for s in range(n_sets):
        parts = hist[[b for b in range(n) if places[b][0] == s]].sum(axis=0) + (key if s == 0 else 0)
        assert np.array_equal(parts, whole[s]), s


def test_a_changed_output_cell_is_a_miss_and_leaves_its_bin(circuit):
    n, adv, sel, tables = circuit
    clean, _ = mm.multiplicities(adv, sel, tables)
    row = int(np.nonzero(sel[5 * 1 + 2])[0][7])  # an S-box row of set 1
    bad = adv.copy()
    bad[3 * 1 + 1, row] ^= 1
    hist, misses = mm.multiplicities(bad, sel, tables)
    assert misses == 1
    diff = clean - hist
    assert diff.sum() == 1 and diff[1, 256 + int(adv[3, row])] == 1
