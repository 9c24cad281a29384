"""What a chip-keeping host does with a VALUES witness, in numpy: fill every cell the layout leaves out by copying.  Uses only the
public layout_index / packed_index / key_packed_index and block_copy_graph -- not the checker's table -- and applies the copy
edges in call order, so it is an expectation independent of aesw_vals_check.h.  The result is a PACKED witness the existing
checkers (the lane model's check_block on the CPU, Context.check_witness on the device) take."""
import numpy as np

AES_ROWS, KEY_ROWS, WORDS_ROWS = 1360, 400, 96
VALUES, PACKED = 2, 1


def reconstruct(pkg, pt, y, z, key_cols, per_block_keys):
    """pt uint8[n,16]; y / z: the VALUES columns (n*448, n*608); key_cols = (w, kx, ky, kz) of one packed key slab, or n with
    per_block_keys.  Returns the PACKED (x, y, z) columns, flat."""
    pt = np.ascontiguousarray(pt, np.uint8).reshape(-1, 16)
    n = pt.shape[0]
    nk = n if per_block_keys else 1
    dense = [np.zeros((n, AES_ROWS), np.uint8) for _ in range(3)]
    dense[0][:, :16] = pt
    for col, src in ((1, y), (2, z)):
        idx = pkg.layout_index(VALUES, col)
        rows = np.nonzero(idx >= 0)[0]
        dense[col][:, rows] = np.asarray(src, np.uint8).reshape(n, -1)[:, idx[rows]]
    w, kx, ky, kz = key_cols
    key = [np.zeros((nk, KEY_ROWS), np.uint8) for _ in range(3)]
    for col, src in enumerate((kx, ky, kz)):
        idx = pkg.key_packed_index(col)
        rows = np.nonzero(idx >= 0)[0]
        key[col][:, rows] = np.asarray(src, np.uint8).reshape(nk, -1)[:nk][:, idx[rows]]
    words = np.asarray(w, np.uint8).reshape(-1, WORDS_ROWS)[:nk]
    for e in pkg.block_copy_graph():  # call order: a source is final before it is read
        assert e["dst_space"] == 0
        sp, sc, sr = int(e["src_space"]), int(e["src_col"]), int(e["src_row"])
        src = dense[sc][:, sr] if sp == 0 else key[sc][:, sr] if sp == 1 else words[:, sr]
        dense[int(e["dst_col"])][:, int(e["dst_row"])] = src
    out = []
    for col in range(3):
        idx = pkg.packed_index(col)
        out.append(np.ascontiguousarray(dense[col][:, idx >= 0]).reshape(-1))
    return tuple(out)
