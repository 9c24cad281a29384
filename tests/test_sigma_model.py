"""The specification of libaesw_sigma.so without a GPU.

csrc/aesw_sigma.h -- the field constants derived from the generator, the cell index, the split of omega's exponent, the sets, the
chunks, the workspace, the column order -- is compiled alone with g++ (tests/sigma_rule_driver.cpp: no ROCm include, no GPU) and
held against tests/sigma_model.py.  The host mapping code runs in a process of its own (tests/sigma_mapping_driver.cpp), once
plain and once under -fsanitize=address,undefined: its mapping equals the model's word for word, is a permutation whose cycles
are exactly the connected components of the placed copy edges (a union-find of the test's own), and maps every other cell to
itself.  The model itself is held against halo2's statement: over the oracle's circuit bytes the closing product is 1, and it
is not after one planted change in a copied cell.  The model's fast form, product_batched, is held equal to the literal product
over every shape of sc.PRODUCTS, planted zero terms, entries out of range and challenges that are not canonical."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sigma_cases as sc
import sigma_model as sm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sigma_rule") / "sigma_rule_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(CSRC), str(ROOT / "tests" / "sigma_rule_driver.cpp"), "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (args, out.stderr)
        return out.stdout.splitlines()
    return run


def test_the_header_is_free_of_hip():
    text = (CSRC / "aesw_sigma.h").read_text()
    assert "hip/" not in text and "asm" not in text.replace("assembly", "").replace("Assembly", "")


def test_the_field_constants_have_their_properties_and_are_the_models(driver):
    g, root, delta = [int(line, 16) for line in driver("constants")]
    assert g == sm.G == 7 and (sm.R - 1) == sm.T << 28 and sm.T % 2 == 1
    assert root == pow(sm.G, sm.T, sm.R) and delta == sm.DELTA
    assert pow(delta, sm.T, sm.R) == 1 and delta != 1
    for k in (10, 14, 15, 17, 20, 28):
        w = int(driver("omega", k)[0], 16)
        assert w == sm.omega(k) and pow(w, 1 << k, sm.R) == 1 and pow(w, 1 << (k - 1), sm.R) == sm.R - 1, k


def test_a_cell_index_decodes_to_its_column_and_row(driver):
    k, n_cols = 12, 5
    probes = (0, 1, 4095, 4096, 4097, 5 * 4096 - 1, 5 * 4096, 0xFFFFFFFF, 3 * 4096 + 77)
    got = [[int(v) for v in line.split()] for line in driver("index", k, n_cols, *probes)]
    assert got == [[m >> k, m & 4095, int(m < n_cols << k), m] for m in probes]
    # 2^32 cells: every index is in range
    assert [int(line.split()[2]) for line in driver("index", 28, 16, 0xFFFFFFFF, 0)] == [1, 1]


@pytest.mark.parametrize("k", (10, 14, 15, 28))
def test_omega_to_a_row_is_the_product_of_a_low_and_a_high_cell(driver, k):
    n = 1 << k
    rows = sorted({0, 1, n - 1, n // 2, 16383 % n, 16384 % n, 16385 % n, (n - 16384) % n, 0x2aaaaaa % n, 0x1555555 % n})
    w = sm.omega(k)
    for i, line in zip(rows, driver("split", k, *rows)):
        lo, hi, value = line.split()
        assert (int(lo), int(hi)) == (i & 16383, i >> 14) and int(lo) < 1 << min(k, 14) and int(hi) < 1 << max(k - 14, 0)
        assert int(value, 16) == pow(w, i, sm.R), (k, i)
    t = sm.tables(k, 3) if k <= 15 else None
    if t:
        at = (0, 1, len(t) - 4, len(t) - 3, len(t) - 2, len(t) - 1, (1 << min(k, 14)) - 1)
        assert [int(line, 16) for line in driver("cell", k, *at)] == [t[a] for a in at]


def test_the_sets_the_chunks_and_the_sizes(driver, pkg):
    lib = pkg.api.load_sigma_library()
    for k, n_cols, chunk_len, n_rows in ((10, 1, 1, 1), (10, 4, 3, 1024), (11, 4, 3, 1024), (11, 5, 2, 1025), (12, 14, 3, 4090), (12, 9, 8, 4096), (20, 14, 3, (1 << 20) - 6),
                                         (28, 16, 8, 1 << 28), (17, 3074, 1, 5)):
        lines = driver("geometry", k, n_cols, chunk_len, n_rows)
        sets, last, chunks, stride, tables, ws = [int(v) for v in lines[0].split()]
        model_sets = sm.sets_of(n_cols, chunk_len)
        assert sets == len(model_sets) == -(-n_cols // chunk_len) and [tuple(int(v) for v in line.split()) for line in lines[1:]] == model_sets
        assert last == min(n_rows, (1 << k) - 1) and chunks == last // 1024 + 1 and stride == (1 << k) // 1024 and chunks <= stride
        assert tables == 32 * len(sm.tables(10, n_cols)) - 32 * 1025 + 32 * ((1 << min(k, 14)) + (1 << max(k - 14, 0))) == int(lib.aesw_sigma_tables_bytes(k, n_cols))
        assert ws == 32 * n_cols + sets * (stride * (32 + 32 + 16) + 64 + 16) == int(lib.aesw_sigma_workspace_bytes(k, n_cols, chunk_len)) and ws % 16 == 0
    for k, n_cols, chunk_len in ((9, 3, 3), (29, 3, 3), (10, 0, 3), (10, 3075, 3), (28, 17, 3), (10, 3, 0), (10, 3, 9)):
        assert [int(v) for v in driver("geometry", k, n_cols, chunk_len, 1)[0].split()][5] == 0 and int(lib.aesw_sigma_workspace_bytes(k, n_cols, chunk_len)) == 0
    assert int(lib.aesw_sigma_tables_bytes(28, 17)) == 0 and int(lib.aesw_sigma_tables_bytes(28, 16)) == 32 * (2 * 16384 + 16)


def test_the_column_order_is_the_configure_order(driver, pkg):
    for n_sets in (1, 2, 5):
        lines = driver("order", n_sets)
        assert int(lines[0]) == sm.columns(n_sets) == pkg.api.permutation_columns(n_sets) == 3 * n_sets + 2
        src = [int(v) for v in lines[1].split()]
        assert src == sm.sources(n_sets) == pkg.api.permutation_sources(n_sets).tolist()
        assert src[:5] == [0, 1, 2, 3 * n_sets, 3 * n_sets + 1] and sorted(src) == list(range(3 * n_sets + 2))  # x0 y0 z0 words rcon, then the other sets
        assert [int(v) for v in lines[2].split()] == [sm.column_of_advice(n_sets, a) for a in range(3 * n_sets + 1)]


# ---- the mapping ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mapping_drivers(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("sigma_mapping")
    lib_dir = ROOT / "halo2-aes_amd"
    exes = []
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = d / ("sigma_mapping_driver_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(CSRC), str(ROOT / "tests" / "sigma_mapping_driver.cpp"), "-o", str(exe),
                        "-L", str(lib_dir), "-laesw", "-Wl,-rpath," + str(lib_dir)], check=True)
        exes.append(exe)

    def run(k, n_sets, n_blocks, sanitized):
        out = d / "map.bin"
        p = subprocess.run([str(exes[sanitized]), str(k), str(n_sets), str(n_blocks), str(out)], capture_output=True, text=True)
        return p.returncode, (np.fromfile(out, np.uint32).reshape(3 * n_sets + 2, 1 << k) if p.returncode == 0 else p.stderr)
    return run


def components(cells, edges):
    """cell -> the smallest cell of its connected component: a union-find of the test's own"""
    parent = {}

    def find(x):
        root = x
        while parent.get(root, root) != root:
            root = parent[root]
        while parent.get(x, x) != x:
            parent[x], x = root, parent[x]
        return root
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return {c: find(c) for c in {v for e in edges for v in e}}


@pytest.mark.parametrize("n_sets", (1, 2))
def test_the_mapping_is_the_models_a_permutation_and_its_cycles_are_the_copy_components(pkg, mapping_drivers, n_sets):
    k = 17
    cap = pkg.block_capacity(k, n_sets)
    key_edges, block_edges = pkg.key_copy_graph(), pkg.block_copy_graph()
    for n_blocks in (0, 1, 3, cap):
        rc, got = mapping_drivers(k, n_sets, n_blocks, False)
        assert rc == 0, got
        if n_blocks in (1, cap):  # the sanitized run: the smallest circuit that has blocks, and the full one
            rc, again = mapping_drivers(k, n_sets, n_blocks, True)
            assert rc == 0 and np.array_equal(again, got), again if rc else "the sanitized build writes another mapping"
        edges = sm.placed_edges(k, n_sets, n_blocks, key_edges, block_edges, lambda b: pkg.api.block_placement(k, n_sets, b))
        assert len(edges) == 640 + 1952 * n_blocks
        assert np.array_equal(got, sm.mapping(k, n_sets, edges)), (n_sets, n_blocks)
        assert np.array_equal(got, pkg.api.permutation_mapping(k, n_sets, n_blocks))
        flat = got.reshape(-1)
        assert np.array_equal(np.sort(flat), np.arange(flat.size, dtype=np.uint32))  # a permutation
        comp = components(flat.size, edges)
        touched = np.array(sorted(comp), np.int64)
        others = np.ones(flat.size, bool)
        others[touched] = False
        assert np.array_equal(flat[others], np.arange(flat.size, dtype=np.uint32)[others])  # every other cell maps to itself
        label = np.arange(flat.size, dtype=np.int64)
        label[touched] = [comp[c] for c in touched]
        assert np.array_equal(label[flat], label)  # sigma stays inside a component ...
        nxt, seen, cycles = flat.tolist(), set(), 0
        for c in comp:  # ... and walks all of it: as many cycles among the touched cells as components
            if c not in seen:
                cycles += 1
                while c not in seen:
                    seen.add(c)
                    c = nxt[c]
        assert cycles == len(set(comp.values())) > 100 and seen == set(comp)
        rcon = sm.column_of_advice(n_sets, 3 * n_sets) + 1
        assert rcon == 4 and np.array_equal(got[rcon], np.arange(rcon << k, (rcon + 1) << k, dtype=np.uint32))  # the fixed column takes part in no copy
    assert mapping_drivers(k, n_sets, cap + 1, False)[0] == 3
    with pytest.raises(pkg.AeswError) as e:
        pkg.api.permutation_mapping(k, n_sets, cap + 1)
    assert e.value.status == pkg.api.ERR_CAPACITY
    for bad in ((9, 1, 0), (29, 1, 0), (17, 0, 0), (17, 1025, 0)):
        with pytest.raises(pkg.AeswError):
            pkg.api.permutation_mapping(*bad)


def test_assembly_copy_keeps_the_larger_cycle_left_and_the_calls_left_on_equal_sizes():
    a = sm.Assembly(8)
    a.copy(0, 1)  # equal sizes: 0 stays the head
    assert a.aux[:2] == [0, 0] and a.mapping[:2] == [1, 0] and a.sizes[0] == 2
    a.copy(2, 0)  # the cycle of 0 is larger: it is "left", 2 joins it
    assert a.aux[2] == 0 and a.sizes[0] == 3 and sorted(a.mapping[:3]) == [0, 1, 2]
    before = list(a.mapping)
    a.copy(1, 2)  # one cycle already: nothing
    assert a.mapping == before
    a.copy(4, 5)
    a.copy(5, 0)  # right is larger: swapped
    assert {a.aux[i] for i in (0, 1, 2, 4, 5)} == {0} and a.sizes[0] == 5
    seen, at = set(), 0
    while at not in seen:
        seen.add(at)
        at = a.mapping[at]
    assert seen == {0, 1, 2, 4, 5}


# ---- the batched model ---------------------------------------------------------------------------------------------------------------
# product_batched is the yardstick of tests/test_gpu_sigma_reach.py, whose shapes product() is too slow for: here the two are held
# equal -- every Z of every set and the report -- which is what lets those tests use it.

CHALLENGES = tuple(sc.seeded(s) for s in sc.CHALLENGE_SEEDS)


@pytest.mark.parametrize("shape", sc.PRODUCTS, ids=lambda s: "k%d-c%d-l%d-u%d" % s)
def test_the_batched_product_is_the_literal_one(shape):
    k, n_cols, chunk_len, n_rows = shape
    _buffers, _source, columns, mapping = sc.world(k, n_cols, n_rows, 0x7369 + sc.PRODUCTS.index(shape))
    literal = sm.product(k, list(columns), mapping, *CHALLENGES, chunk_len, n_rows)
    assert not literal[1]["open"] and literal[1]["zero_terms"] == 0
    assert sm.product_batched(k, list(columns), mapping, *CHALLENGES, chunk_len, n_rows) == literal


def test_the_batched_product_is_the_literal_one_over_planted_zero_terms():
    k, n_cols, chunk_len, n_rows = 10, 7, 3, 1018
    cells = ((4, 301), (5, 303), (3, 304), (1, 0), (6, 1017), (6, 500))  # in one lane's rows, at a lane's first row, the first and the last row
    *_, columns, mapping, gamma = sc.planted_zeros(k, sc.world(k, n_cols, n_rows, 0x737a), cells, (0, 700), CHALLENGES[0])
    literal = sm.product(k, list(columns), mapping, CHALLENGES[0], gamma, chunk_len, n_rows)
    assert literal[1]["zero_terms"] == len(cells) and literal[1]["first_zero"] == 0 and literal[1]["open"]
    assert literal[0][0][0] == 1 and not any(literal[0][0][1:]) and not any(literal[0][1]) and not any(literal[0][2])
    assert sm.product_batched(k, list(columns), mapping, CHALLENGES[0], gamma, chunk_len, n_rows) == literal
    # without the zero at row 0 the sets in front of the first zero keep their values
    *_, columns, mapping, gamma = sc.planted_zeros(k, sc.world(k, n_cols, n_rows, 0x737a), cells[:3], (0, 700), CHALLENGES[0])
    literal = sm.product(k, list(columns), mapping, CHALLENGES[0], gamma, chunk_len, n_rows)
    assert literal[1]["zero_terms"] == 3 and literal[1]["first_zero"] == (1 << k) + 301 and all(literal[0][0]) and all(literal[0][1][:302]) and not any(literal[0][1][302:])
    assert sm.product_batched(k, list(columns), mapping, CHALLENGES[0], gamma, chunk_len, n_rows) == literal


def test_the_batched_product_is_the_literal_one_over_entries_out_of_range_and_challenges_that_are_not_canonical():
    k, n_cols, chunk_len, n_rows = 10, 5, 2, 1018
    _buffers, _source, columns, mapping = sc.world(k, n_cols, n_rows, 0x736f)
    mapping = mapping.copy()
    mapping[3, 500] = n_cols * (1 << k) + 5
    mapping[0, 0] = 0xFFFFFFFF
    mapping[4, 1020] = 0xFFFFFFFF  # at a row behind n_rows: neither read nor counted
    cols = list(columns)
    cols[2] = None  # a column that reads as zero bytes
    literal = sm.product(k, cols, mapping, *CHALLENGES, chunk_len, n_rows)
    assert literal[1]["out_of_range"] == 2 and not literal[1]["noncanonical"]
    assert sm.product_batched(k, cols, mapping, *CHALLENGES, chunk_len, n_rows) == literal
    for beta, gamma in ((sc.NONCANONICAL[0], CHALLENGES[1]), (CHALLENGES[0], sc.NONCANONICAL[1])):
        literal = sm.product(k, cols, mapping, beta, gamma, chunk_len, n_rows)
        assert literal[1]["noncanonical"] and literal[1]["out_of_range"] == 2
        assert sm.product_batched(k, cols, mapping, beta, gamma, chunk_len, n_rows) == literal


def test_the_models_closing_product_is_one_over_the_oracles_circuit_and_not_after_a_change(pkg, oracle):
    k, n_sets, n = 17, 1, 3
    rng = np.random.default_rng(0x7369676d61)
    key, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
    with oracle.circuit(k, n_sets, key, pt, record_copies=False) as c:
        assert c.status == 0
        adv = np.stack([c.advice(i) for i in range(3 * n_sets + 1)])
    _sel, fixed = pkg.assemble_selectors(k, n_sets, n)
    buffers = np.concatenate([adv, np.asarray(fixed, np.uint8).reshape(1, -1)])
    cols = [buffers[s] for s in sm.sources(n_sets)]
    mapping = pkg.api.permutation_mapping(k, n_sets, n)
    beta, gamma = 0x1234567890abcdef1234567890abcdef % sm.R, 0xfedcba0987654321fedcba0987654321 % sm.R
    u = (1 << k) - 6
    assert sm.closing_ratio(k, cols, mapping, beta, gamma, u) == 1
    c_, i = next((c_, i) for c_ in range(5) for i in range(400, 2000) if mapping[c_, i] != (c_ << k) + i)  # a copied cell of the first block
    cols[c_] = cols[c_].copy()
    cols[c_][i] ^= 1
    assert sm.closing_ratio(k, cols, mapping, beta, gamma, u) != 1
