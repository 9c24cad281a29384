"""The options of aesw_set_option / aesw_get_option as they have always been, written out (a helper module, not a conftest), and
the driver that dumps csrc/aesw_options.h's table for comparison.

EXPECTED was written from the strcmp chains of aesw_set_option / aesw_get_option and the field initialisers of aesw_ctx.h as they
stood before the table existed: name -> (default, lowest, highest, form, settable, readable).  `default` is what a fresh context
with the reference tables reads (None: set-only, or it depends on the machine); lowest / highest are None for a name that cannot
be set.  tests/test_option_table.py holds the table against it without a GPU, tests/test_gpu_options.py a real context."""
import subprocess
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

Row = namedtuple("Row", "default lo hi form settable readable")
_RW = lambda default, lo, hi, form="range": Row(default, lo, hi, form, True, True)  # noqa: E731
_RO = lambda default: Row(default, None, None, "range", False, True)               # noqa: E731

EXPECTED = {
    "waves_shared": _RW(0, 0, 4),
    "waves_pbk": _RW(0, 0, 4),
    "nt_stores": _RW(1, I64_MIN, I64_MAX, "truthy"),  # any value: stores value != 0 into "store_mode", reads "store_mode" == 1
    "store_mode": _RW(1, 0, 2),
    "key_store_mode": _RW(1, 0, 2),
    "fr_geometry": _RW(1, 0, 2),
    "fr_store_mode": _RW(1, 0, 2),
    "assemble_geometry": _RW(4, 0, 4),
    "grid_cap": _RW(0, 0, 0x7fffffff),
    "xcd_remap": _RW(1, 0, 1 << 24),
    "lds_pad": _RW(0, 0, 120 * 1024),
    "arena_align_log2": _RW(0, 7, 32, "zero_or_range"),  # 0, or 7 ... 32
    "arena_probe": _RW(-1, -1, 64),
    "arena_unit": _RW(2, 0, 2),
    "trace_ptr": Row(None, I64_MIN, I64_MAX, "range", False, False),  # -DAESW_TRACE builds only (set-only there)
    "force_table_path": _RW(0, I64_MIN, I64_MAX),  # one way: a non-zero value switches the context to the table path for good
    "chunk_blocks": _RW(1 << 15, 64, I64_MAX),
    "batch_streams": _RW(3, 1, 8),
    "copy_threads": _RW(-1, -1, 64),
    "key_slots": _RW(4, 1, 64),
    "split_small": _RW(0, 0, 8),
    "stream_check": _RW(0, 0, 1),
    "stream_poison": _RW(0, 0, I64_MAX),
    "arena_cache": _RW(1, 0, 1),
    "arena_cache_max_mb": _RW(65536, 0, 1 << 30),
    "arena_probe_budget_ms": _RW(3000, 0, 600000),
    "effective_waves_shared": _RO(3),
    "effective_waves_pbk": _RO(1),
    "effective_waves_key": _RO(3),
    "effective_copy_threads": _RO(None),  # a share of the CPUs the process may run on
    "arena_cache_hits": _RO(0),
    "arena_cached_bytes": _RO(0),
    "key_reader_waits": _RO(0),
    "key_writer_waits": _RO(0),
    "key_slots_allocated": _RO(1),  # the slot aesw_create makes
    "key_slots_pinned": _RO(0),
}
BUILD_ONLY = {"trace_ptr"}
# names whose value is not a field of AeswOptions (the driver has no default to dump for them)
FIELDLESS = {"trace_ptr", "force_table_path", "key_slots"} | {n for n, r in EXPECTED.items() if not r.settable}
ALIASES = (("nt_stores", "store_mode"),)  # two names, one field


def outside(row):
    """Values next to a settable row's range that must be refused (none for a row that takes any value)."""
    if row.form == "truthy":
        return []
    vals = [row.lo - 1, row.hi + 1]
    if row.form == "zero_or_range":
        vals += [-1, 1]  # below the 0, and between the 0 and the range
    return [v for v in vals if I64_MIN <= v <= I64_MAX]


def inside(row):
    """Lowest and highest accepted value (and the 0 of a zero_or_range row)."""
    return [row.lo, row.hi] + ([0] if row.form == "zero_or_range" else [])


def build_driver(directory) -> Path:
    """g++ tests/option_table_driver.cpp against csrc/aesw_options.h alone."""
    exe = Path(directory) / "option_table_driver"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "halo2-aes_amd" / "csrc"),
                    str(ROOT / "tests" / "option_table_driver.cpp"), "-o", str(exe)], check=True)
    return exe


def dump(exe):
    """The table's rows as the driver prints them: name -> (Row, build_only); default None where the row has no field."""
    rows = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        name, default, lo, hi, form, s, g, b = line.split()
        assert name not in rows, name
        rows[name] = (Row(None if default == "-" else int(default), int(lo), int(hi), form, s == "1", g == "1"), b == "1")
    return rows


def drive(exe, script):
    """Runs ("s", name, value) / ("g", name) commands on one AeswOptions; per command None (refused), True (set) or the value read."""
    text = "\n".join(" ".join(str(v) for v in cmd) for cmd in script)
    out = subprocess.run([str(exe), "script"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(script)
    return [None if line == "refused" else (True if line == "ok" else int(line.split()[1])) for line in out]
