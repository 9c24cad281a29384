"""The lookup multiplicities of a VALUES witness restated in numpy.  It knows three things and nothing of the kernel: the table of
aesw_vals_check_table (which cell each operand of a block's 1 056 lookups is), the image those offsets address (include/aesw_vals.h:
y | z | pt | kx | ky | kz | words_column), and aesw_mult_bin.  A lookup is a hit when its output is what the table row its inputs
name holds (z == x ^ y on an xor row, y == table[tag - 3][x] otherwise); a miss is counted in no bin.  Held against
tests/mult_model.py over the oracle's circuit in tests/test_vacc_model.py."""
import numpy as np

BINS = 66561
O_Z, O_PT, O_KX, O_KY, O_KZ, O_W, IMAGE = 448, 1056, 1072, 1472, 1712, 1912, 2008


def images(pt, y, z, kz, w):
    """uint8[n, 2008]: the image of every block (kx and ky stay 0: no lookup of a block reads them)."""
    pt = np.asarray(pt, np.uint8).reshape(-1, 16)
    n = pt.shape[0]
    img = np.zeros((n, IMAGE), np.uint8)
    img[:, :O_Z] = np.asarray(y, np.uint8).reshape(n, 448)
    img[:, O_Z:O_PT] = np.asarray(z, np.uint8).reshape(n, 608)
    img[:, O_PT:O_KX] = pt
    img[:, O_KZ:O_W] = np.asarray(kz, np.uint8).reshape(-1)[:200]
    img[:, O_W:] = np.asarray(w, np.uint8).reshape(-1)[:96]
    return img


def multiplicities(pkg, k, n_sets, first_block, pt, y, z, kz, w, tables):
    """-> (hist int64[n_sets, 66561], report dict as api.mult_report_dict gives it) of blocks first_block ... of the circuit."""
    words, rows = pkg.api.vals_check_table()
    assert pkg.api.load_vals_library().aesw_vals_image_bytes() == IMAGE
    ox, oy, oz, tag = words[:, 0] & 0xFFFF, words[:, 0] >> 16, words[:, 1] & 0xFFFF, (words[:, 1] >> 16).astype(np.int64)
    xor = tag == 2
    img = images(pt, y, z, kz, w).astype(np.int64)
    n = img.shape[0]
    x, yy = img[:, ox], img[:, oy]
    zz = img[:, np.where(xor, oz, 0)]
    looked = np.stack([np.asarray(t, np.int64) for t in tables])[np.where(xor, 0, tag - 3)[None, :], x]
    hit = np.where(xor[None, :], zz == (x ^ yy), yy == looked)
    bin_of = pkg.api.load_mult_library().aesw_mult_bin  # asked once per distinct (tag, x, y); a one-operand tag ignores y
    keys = (np.broadcast_to(tag[None, :], x.shape) << 16) | (x << 8) | np.where(xor[None, :], yy, 0)
    uniq, inverse = np.unique(keys, return_inverse=True)
    bins = np.array([int(bin_of(int(u) >> 16, (int(u) >> 8) & 0xFF, int(u) & 0xFF)) for u in uniq], np.int64)[inverse].reshape(x.shape)
    hist = np.zeros((n_sets, BINS), np.int64)
    first = None
    for i in range(n):
        s, _row = pkg.block_placement(k, n_sets, first_block + i)
        hist[s] += np.bincount(bins[i][hit[i]], minlength=BINS)
        if first is None and not hit[i].all():
            first = (first_block + i, False, int(rows[np.nonzero(~hit[i])[0][0]]))
    return hist, {"lookups": 1056 * n, "misses": int((~hit).sum()), "first_miss": first}
