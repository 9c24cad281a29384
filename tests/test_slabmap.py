"""The slab map (csrc/aesw_slabmap.h: row -> tag, tag -> assigned / kept cells, and what is counted from those) against its two
independent restatements.  No GPU, no ROCm include:

  * the header compiles alone with g++ -fsyntax-only, which also evaluates every static_assert in it (the copy counts, the
    closed-form packed indices against the prefix counts of the classifiers);
  * tests/slabmap_dump.cpp, built against csrc/, prints every derived table;
  * the masks, packed indices, strides and copy counts are held against tests/slab_map.py (one block and one key slab written
    row by row from the table of DESIGN.md 2), the tags, the values mask and words_column's gate -- which slab_map.py does not
    state -- against the selectors and masks of the oracle's circuit."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import slab_map

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
DENSE, PACKED, VALUES = 0, 1, 2


def test_header_stands_alone():
    """aesw_slabmap.h needs nothing but <stdint.h>, and its static_asserts hold."""
    text = (CSRC / "aesw_slabmap.h").read_text()
    assert re.findall(r"^\s*#\s*include\s+(\S+)", text, re.M) == ["<stdint.h>"]
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-x", "c++", "-"],
                   input='#include "aesw_slabmap.h"\n', text=True, check=True)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """{(table name, argument): its values as an int array} for the tables the dump program prints in full."""
    exe = tmp_path_factory.mktemp("slabmap") / "slabmap_dump"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(CSRC), str(ROOT / "tests" / "slabmap_dump.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    tables = {}
    for ln in out.splitlines():
        head, _, body = ln.partition(":")
        name, arg = head.split()
        if "fnv1a" not in body and "<" not in body:
            tables[name, int(arg)] = np.array(body.split(), np.int64)
        elif "<" in body:
            tables[name, int(arg)] = body.split()
    return tables


@pytest.fixture(scope="module")
def restated(oracle):
    """slab_map.py's one key slab and one block: (ymask, zmask) of the block, of the key slab, and words_column."""
    sbox, mul2, mul3 = oracle.fips_tables()
    rng = np.random.default_rng(5)
    rk, words, _kx, _ky, _kz, kym, kzm = slab_map.key_schedule(rng.integers(0, 256, 16, dtype=np.uint8), sbox)
    _x, _y, _z, ym, zm, _ct = slab_map.encrypt_slab(rng.integers(0, 256, 16, dtype=np.uint8), rk, sbox, mul2, mul3)
    return (np.asarray(ym, bool), np.asarray(zm, bool)), (np.asarray(kym, bool), np.asarray(kzm, bool)), np.asarray(words)


def prefix_index(mask):
    return np.where(mask, np.cumsum(mask) - 1, -1)


def test_masks_indices_and_strides_match_the_restated_slabs(dump, restated, oracle):
    (ym, zm), (kym, kzm), words = restated
    enc = [np.ones(1360, bool), ym, zm]
    key = [np.ones(400, bool), kym, kzm]
    for c in range(3):
        assert np.array_equal(dump["encrypt_assigned_mask", c], enc[c])
        assert np.array_equal(dump["key_assigned_mask", c], key[c])
        assert np.array_equal(dump["encrypt_assigned_mask", c], oracle.assigned_mask(c))
        assert np.array_equal(dump["key_assigned_mask", c], oracle.key_assigned_mask(c))
        assert np.array_equal(dump["encrypt_values_mask", c], oracle.values_mask(c))
        assert np.array_equal(dump["packed_index_enc", c], prefix_index(enc[c]))
        assert np.array_equal(dump["packed_index_key", c], prefix_index(key[c]))
    # a stride is the number of cells the layout keeps; a values cell is a y that no xor row holds, or a z
    kstr = [400, kym.sum(), kzm.sum()]
    assert list(dump["slab_strides", DENSE]) == [1360, 1360, 1360, len(words), 400, 400, 400]
    assert list(dump["slab_strides", PACKED]) == [1360, ym.sum(), zm.sum(), len(words)] + kstr
    assert list(dump["slab_strides", VALUES]) == [0, (ym & ~zm).sum(), zm.sum(), len(words)] + kstr
    assert list(dump["slab_strides", PACKED]) == [1360, 1056, 608, 96, 400, 240, 200]
    assert list(dump["slab_strides", VALUES])[:3] == [0, 448, 608]
    # one copy_advice() per x cell below the plaintext rows and per y cell of an xor row; 4 shifted words_column rows a key round
    assert len(dump["block_copy_graph", 1952]) == (1360 - 16) + zm.sum() == 1952
    assert len(dump["key_copy_graph", 640]) == 400 + kzm.sum() + 4 * 10 == 640


def test_tags_match_the_selectors_of_the_oracle_circuit(dump, restated, oracle):
    _enc, _key, words = restated
    etag, ktag = dump["encrypt_selector_tags", 0], dump["key_selector_tags", 0]
    q, rc = dump["q_eq_rcon", 0], dump["rcon_fixed", 0]
    rng = np.random.default_rng(6)
    with oracle.circuit(12, 1, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, (1, 16), dtype=np.uint8),
                        record_copies=False) as c:
        expect = np.zeros(c.num_rows, np.int64)
        expect[:400] = ktag
        assert c.block_placement(0) == (0, 400)
        expect[400:1760] = etag
        for tag in range(1, 6):  # selectors of set 0: range, xor, sbox, mul2, mul3
            assert np.array_equal(c.selector(tag - 1), (expect == tag).astype(np.uint8)), "tag %d" % tag
        q_sel = c.selector(5)
        assert np.array_equal(q_sel[:96], q) and not q_sel[96:].any()
        assert np.array_equal(c.fixed()[:96], rc)
    # the cell rule on those tags is the masks: y iff tag >= 2, z iff tag == 2; VALUES: y iff tag >= 3
    assert np.array_equal(dump["encrypt_assigned_mask", 1], etag >= 2) and np.array_equal(dump["encrypt_assigned_mask", 2], etag == 2)
    assert np.array_equal(dump["key_assigned_mask", 1], ktag >= 2) and np.array_equal(dump["key_assigned_mask", 2], ktag == 2)
    assert np.array_equal(dump["encrypt_values_mask", 1], etag >= 3) and np.array_equal(dump["encrypt_values_mask", 2], etag == 2)
    # the round constants sit where slab_map.py's words_column has them
    rows = np.flatnonzero(q)
    assert list(rows) == [20 + 8 * rho for rho in range(10)] and np.array_equal(rc[rows], words[rows]) and list(rc[rows]) == slab_map.RCON
    assert not rc[q == 0].any()
