"""The cut rule of the multiplicity accumulator restated in numpy: a run of a circuit's blocks -> one piece per column set it
touches -> chunks of at most `chunk` blocks, and what one chunk contributes by tests/mult_model.py.  The only thing taken from
the product is the capacity function (aesw_block_capacity, pure host).  Held against the oracle's circuit in
tests/test_acc_model.py; the GPU tests take their expected histograms from mult_model over the whole circuit, not from here."""
import numpy as np

AES_ROWS, KEY_ROWS = 1360, 400


def set_firsts(capacity, k, n_sets):
    """[n_sets + 1]: the circuit-local index of the first block of every set, then the circuit's capacity."""
    return [0] + [int(capacity(k, s)) for s in range(1, n_sets + 1)]


def cut(firsts, first_block, n_blocks, chunk):
    """[(set, first block, blocks)]: blocks [first_block, first_block + n_blocks) cut at the set boundaries, every piece cut
    into chunks of `chunk` blocks (the last one of a piece may be shorter)."""
    end, out = first_block + n_blocks, []
    assert 0 <= first_block and end <= firsts[-1] and chunk >= 1
    for s in range(len(firsts) - 1):
        lo, hi = max(first_block, firsts[s]), min(end, firsts[s + 1])
        out += [(s, b, min(chunk, hi - b)) for b in range(lo, hi, chunk)]
    return out


def rows_of(firsts, s, block, count):
    """The circuit rows of `count` blocks of set s from circuit block `block` on: set 0's blocks lie behind the key rows."""
    r0 = (KEY_ROWS if s == 0 else 0) + (block - firsts[s]) * AES_ROWS
    return slice(r0, r0 + count * AES_ROWS)


def masked(selectors, s, rows):
    """The selector columns with only set s's five lookup selectors left on, and those only on `rows`."""
    out = np.zeros_like(selectors)
    out[5 * s:5 * s + 5, rows] = selectors[5 * s:5 * s + 5, rows]
    return out


def chunk_contribution(mm, advice, selectors, tables, firsts, piece):
    s, block, count = piece
    return mm.multiplicities(advice, masked(selectors, s, rows_of(firsts, s, block, count)), tables)


def key_contribution(mm, advice, selectors, tables):
    return mm.multiplicities(advice, masked(selectors, 0, slice(0, KEY_ROWS)), tables)
