"""The case table of tests/test_gpu_instantiations.py, and the kernel instantiations it launches.

Imports without a GPU (numpy-free, no torch): tests/test_instantiation_coverage.py derives from these tables, through the
dispatch rules of aesw_api.cpp / aesw_kernels.hip restated below, the set of template instantiations the sweep launches and
holds it against the kernels libaesw.so carries.  A dispatch rule changed in the C++ must be changed here too, or the
coverage test (or the sweep's kernel trace) disagrees."""

DENSE, PACKED, VALUES = 0, 1, 2
LAYOUTS = (DENSE, PACKED, VALUES)
LAYOUT_NAME = {DENSE: "dense", PACKED: "packed", VALUES: "values"}
KM_PBK, KM_SHARED, KM_PRE = 0, 1, 2                   # encrypt_kernel's KM (aesw_encrypt_witness_device)
KEY_FORMS = ("scheduled", "shared", "pbk", "pbk_slab")  # pbk_slab: per-block keys whose key slab is emitted (KEMIT)
TABLE_PATHS = ("xtime", "generic")                      # encrypt_kernel / key_kernel XT = true / false
STORE_MODES = (0, 1, 2)                                 # "store_mode" / "key_store_mode" / "fr_store_mode" -> NT
DEFAULT_KEY_STORE_MODE = 1
DEFAULT_STORE_MODE = 1
BPW = 16                                                # blocks per wave

# ---- dispatch rules --------------------------------------------------------------------------------------------------


def max_waves(layout):
    """auto_waves' clamp: a group's staging must stay below 64 KiB."""
    return {DENSE: 2, PACKED: 3, VALUES: 4}[layout]


def auto_waves(layout, pbk, waves_shared=0, waves_pbk=0):
    """aesw_api.cpp auto_waves: waves per encrypt_kernel group."""
    if pbk:
        w = waves_pbk or 1
    else:
        w = waves_shared or (2 if layout == DENSE else 3)
    return min(w, max_waves(layout))


def auto_waves_key(layout, want_rk, waves_pbk=0):
    """aesw_api.cpp auto_waves_key: waves per key_kernel group (not clamped by layout)."""
    if waves_pbk:
        return waves_pbk
    if layout == DENSE:
        return 2
    return 4 if want_rk else 3


def key_layout(layout):
    """launch_key: VALUES key slabs are PACKED ones."""
    return DENSE if layout == DENSE else PACKED


def effective_remap(grid_cap, xcd_remap):
    """launch_encrypt drops the remap when striding workgroups would change XCD class (grid_cap % 8 != 0)."""
    return xcd_remap if grid_cap == 0 or grid_cap % 8 == 0 else 0


def assemble_kernel_choice(as_fr, geometry, k, col_count):
    """aesw_layout.h assemble_kernel_choice: 0 striding, 1 one-shot segment grid, 2 aligned one-shot."""
    if not as_fr or col_count == 0:
        return 0
    if geometry == 1:
        segs = 1 + ((1 << k) + 1360 - 1) // 1360
        return 1 if segs <= 65535 and col_count <= 65535 else 0
    if geometry >= 2:
        return 2 if 8 <= k <= 30 and col_count <= 65535 else 0
    return 0


def _b(v):
    return "true" if v else "false"


def encrypt_kernel(layout, xt, form, nt):
    km = {"scheduled": KM_PRE, "shared": KM_SHARED, "pbk": KM_PBK, "pbk_slab": KM_PBK}[form]
    return "encrypt_kernel<%d,%s,%d,%s,%d>" % (layout, _b(xt), km, _b(form == "pbk_slab"), nt)


def key_kernel(layout, xt, nt):
    return "key_kernel<%d,%s,%d>" % (key_layout(layout), _b(xt), nt)


def check_kernel(layout, pbk):
    return "check_kernel<%d,%s>" % (layout, _b(pbk))


def assemble_kernel(geometry, nt, as_fr, k, n_sets):
    choice = assemble_kernel_choice(as_fr, geometry, k, 3 * n_sets + 1)
    if choice == 1:
        return "assemble_fr_oneshot_kernel<%d>" % nt
    if choice == 2:
        pieces, threads = {2: (1, 256), 3: (2, 256)}.get(geometry, (2, 128))
        return "assemble_fr_aligned_kernel<%d,%d,%d>" % (nt, pieces, threads)
    return "assemble_kernel<true,%d>" % nt if as_fr else "assemble_kernel<false,0>"


def expand_kernel(geometry, nt):
    return "expand_fr_kernel<%d>" % nt if geometry == 0 else "expand_fr_oneshot_kernel<%d,%d>" % (nt, geometry)


# ---- the sweep's cases -------------------------------------------------------------------------------------------------

# encrypt: one case per instantiation; inside it every wave count the layout allows, sizes around the group size
ENCRYPT_CASES = [(layout, xt, form, nt) for layout in LAYOUTS for xt in (True, False) for form in KEY_FORMS for nt in STORE_MODES]


def encrypt_sizes(waves):
    g = BPW * waves
    return sorted({1, 15, 16, 17, g - 1, g, g + 1, 3 * g + 5})


# key_kernel: inside each case want_rk x waves_pbk, sizes around the group size, xcd_remap rotated across sizes
KEY_CASES = [(layout, xt, nt) for layout in LAYOUTS for xt in (True, False) for nt in STORE_MODES]
KEY_WAVES_PBK = (0, 1, 2, 3, 4)
KEY_REMAPS = (0, 1, 3)


def key_sizes(waves):
    g = BPW * waves
    return sorted({1, 15, 16, 17, g - 1, g, g + 1, 9 * g + 7})


# striding and remap: every grid_cap x xcd_remap, every key form, packed / values at their default waves and dense at 2
STRIDE_CASES = [(cap, remap) for cap in (1, 3, 8, 24) for remap in (0, 1, 2, 7)]
STRIDE_LAYOUTS = ((PACKED, 0), (VALUES, 0), (DENSE, 2))  # (layout, waves option; 0 = auto)
LDS_PAD = 8192


def stride_group_counts(grid_cap, xcd_remap):
    """Group counts below one turn of 8*C groups, on one whole turn, and one turn plus a tail."""
    per = 8 * max(effective_remap(grid_cap, xcd_remap), 1)
    return (per - 3, per, per + 5)


# assemble: K / N / spare slots of test_gpu_round4's boundary test, every geometry x store flavour x {bytes, Fr}
ASSEMBLE_SHAPES = ((7, 2, 0), (8, 2, 0), (9, 1, 0), (11, 2, 0), (16, 3, 20))
ASSEMBLE_GEOMETRIES = (0, 1, 2, 3, 4)
EXPAND_CASES = [(geo, nt) for geo in (0, 1, 2) for nt in STORE_MODES]
EXPAND_SIZES = (1, 255, 4097)

# host entry point aesw_encrypt_witness: per-block keys with key slab and ct, chunked
HOST_CASES = [(layout, threads, pinned) for layout in LAYOUTS for threads in (1, 4) for pinned in (False, True)]
HOST_CHUNK = 1000
HOST_N = 2 * HOST_CHUNK + 77

# not launched by the sweep, with the reason
EXEMPT = {
    "probe_fill_kernel": "arena probe: fills scratch memory whose values are garbage by design (test_gpu_round3 arena tests)",
    "probe_fronts_kernel": "arena probe: times memory fronts, output is garbage by design (test_gpu_round3 arena tests)",
}


def launched():
    """Every kernel instantiation the sweep's cases launch, named as `nm -C` shows them (spaces removed)."""
    out = set()
    for layout, xt, form, nt in ENCRYPT_CASES:
        out.add(encrypt_kernel(layout, xt, form, nt))
        if form in ("scheduled", "shared"):  # schedule_key / the fused shared-key slab: one key_kernel launch
            out.add(key_kernel(layout, xt, DEFAULT_KEY_STORE_MODE))
        if layout != VALUES:                 # check_witness on the case's output
            out.add(check_kernel(layout, form.startswith("pbk")))
    for layout, xt, nt in KEY_CASES:
        out.add(key_kernel(layout, xt, nt))
    for layout, _w in STRIDE_LAYOUTS:
        for form in KEY_FORMS:
            out.add(encrypt_kernel(layout, True, form, DEFAULT_STORE_MODE))
    for k, n_sets, _spare in ASSEMBLE_SHAPES:
        for geo in ASSEMBLE_GEOMETRIES:
            for nt in STORE_MODES:
                for as_fr in (False, True):
                    out.add(assemble_kernel(geo, nt, as_fr, k, n_sets))
    for geo, nt in EXPAND_CASES:
        out.add(expand_kernel(geo, nt))
    out.add("table_kernel")
    for layout, _t, _p in HOST_CASES:
        out.add(encrypt_kernel(layout, True, "pbk_slab", DEFAULT_STORE_MODE))
    return out
