"""Builds the product libraries in-tree.

  halo2-aes_amd/libaesw.so        HIP kernels + the C ABI of include/aesw.h (hipcc --offload-arch=gfx950)
  halo2-aes_amd/libaesw_host.so   the C++ mirror of the reference's host interface (include/aesw_host.h): plain g++,
                                  no device code, linked against libaesw.so -- it only calls the C ABI
  halo2-aes_amd/libaesw_circ.so   the many-circuit witness checker of include/aesw_circ.h: one more gfx950 kernel and its
                                  entry point (hipcc), linked against libaesw.so, whose context it takes
  halo2-aes_amd/libaesw_cols.so   the checker of the assembled advice columns, bytes or Fr cells (include/aesw_cols.h): built and
                                  linked like libaesw_circ.so
  halo2-aes_amd/libaesw_vals.so   the checker of a VALUES witness (include/aesw_vals.h): built and linked like libaesw_circ.so

hipcc cross-compiles gfx950 code objects without a GPU.  The .so is git-ignored
but travels to the GPU box with the snapshot.  (The test-only artefacts are
built by __graft_entry__.build(), not from inside the product package.)
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB = PKG / "libaesw.so"
HOST_LIB = PKG / "libaesw_host.so"
CIRC_LIB = PKG / "libaesw_circ.so"
COLS_LIB = PKG / "libaesw_cols.so"
VALS_LIB = PKG / "libaesw_vals.so"


def _newer(target: Path, sources) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(Path(s).stat().st_mtime <= t for s in sources)


def _run(cmd, cwd=None):
    proc = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError("build failed: %s\n%s" % (" ".join(map(str, cmd)), proc.stdout))
    return proc.stdout


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found")


def _build(target: Path, deps, command, force: bool) -> Path:
    """`target` from `deps`, unless it is newer than all of them and not forced.  `command(tmp)` is the argument list that writes
    the library to `tmp`.  Several ranks may get here at once (torchrun): serialise on a lock file, look again (another process
    may have built it while we waited), build under a private name, publish with an atomic rename."""
    if not force and _newer(target, deps):
        return target
    import fcntl
    with open(PKG / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and _newer(target, deps):
                return target
            tmp = target.with_suffix(".so.tmp%d" % os.getpid())
            _run(command(tmp))
            os.replace(tmp, target)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return target


def build_host(force: bool = False) -> Path:
    """libaesw_host.so: host code only (g++), NEEDED libaesw.so found next to it ($ORIGIN)."""
    host = PKG / "host"
    srcs = [host / "host_capi.cpp"]
    deps = srcs + [ROOT / "include" / "aesw.h", ROOT / "include" / "aesw_host.h", host / "halo2_lite.hpp", host / "aes_gadget.hpp", LIB]
    return _build(HOST_LIB, deps, lambda tmp: ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", str(tmp)] + [str(s) for s in srcs] +
                  ["-L" + str(PKG), "-laesw", "-Wl,-rpath,$ORIGIN"], force)


# The one list of what libaesw.so is made of: tools that build a private variant of the library (tools/trace.py, parts.py,
# key_ab.py, sanitize.sh) take it from here.
PRODUCT_SOURCES = [CSRC / n for n in ("aesw_kernels.hip", "aesw_api.cpp", "aesw_keyring.cpp", "aesw_hostpath.cpp", "aesw_arena.cpp",
                                      "aesw_comm.cpp", "aesw_group.cpp", "aesw_circuits.cpp")]
PRODUCT_HEADERS = [CSRC / n for n in ("aesw_lane.h", "aesw_layout.h", "aesw_check.h", "aesw_check_dev.h", "aesw_internal.h", "aesw_ctx.h",
                                      "aesw_keyring.h")] + \
    [ROOT / "include" / "aesw.h"]


# csrc/ itself holds exactly the sources of libaesw.so (PRODUCT_SOURCES); the second library's live one level down
CIRC_SOURCES = [CSRC / "circ" / "aesw_circ_check.hip"]
CIRC_HEADERS = [CSRC / n for n in ("aesw_check_dev.h", "aesw_circ_search.h", "aesw_check.h", "aesw_layout.h", "aesw_internal.h", "aesw_ctx.h",
                                   "aesw_keyring.h")] + \
    [ROOT / "include" / "aesw.h", ROOT / "include" / "aesw_circ.h"]


def _checker_command(sources):
    """libaesw_circ.so, libaesw_cols.so and libaesw_vals.so are built and linked alike."""
    return lambda tmp: [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread", "-o", str(tmp)] + \
        [str(s) for s in sources] + ["-L" + str(PKG), "-laesw", "-Wl,-rpath,$ORIGIN"]


def build_circ(force: bool = False) -> Path:
    """libaesw_circ.so: the many-circuit checker kernel and its entry point (hipcc, gfx950), NEEDED libaesw.so found next to it
    ($ORIGIN).  A library of its own: the set of kernels inside libaesw.so stays what it is."""
    return _build(CIRC_LIB, CIRC_SOURCES + CIRC_HEADERS + [LIB], _checker_command(CIRC_SOURCES), force)


COLS_SOURCES = [CSRC / "cols" / "aesw_cols_check.hip"]
COLS_HEADERS = CIRC_HEADERS[:-1] + [ROOT / "include" / "aesw_cols.h"]


def build_cols(force: bool = False) -> Path:
    """libaesw_cols.so: the checker of the assembled advice columns and its entry point (hipcc, gfx950), NEEDED libaesw.so found
    next to it ($ORIGIN).  A library of its own, like libaesw_circ.so: the kernel sets of the other two stay what they are."""
    return _build(COLS_LIB, COLS_SOURCES + COLS_HEADERS + [LIB], _checker_command(COLS_SOURCES), force)


VALS_SOURCES = [CSRC / "vals" / "aesw_vals_check.hip"]
VALS_HEADERS = [h for h in CIRC_HEADERS[:-1] if h.name != "aesw_circ_search.h"] + [CSRC / "aesw_vals_check.h", ROOT / "include" / "aesw_vals.h"]


def build_vals(force: bool = False) -> Path:
    """libaesw_vals.so: the checker of a VALUES witness and its entry point (hipcc, gfx950), NEEDED libaesw.so found next to it
    ($ORIGIN).  A library of its own, like libaesw_circ.so and libaesw_cols.so: the kernel sets of the other three stay what they are."""
    return _build(VALS_LIB, VALS_SOURCES + VALS_HEADERS + [LIB], _checker_command(VALS_SOURCES), force)


def build_product(force: bool = False, extra_flags=(), out: Path = LIB, extra_sources=()) -> Path:
    """libaesw.so, or with `extra_flags` / `extra_sources` and another `out` a diagnostic variant of it (-DAESW_TRACE, ...)."""
    srcs = PRODUCT_SOURCES + [Path(s) for s in extra_sources]
    return _build(Path(out), srcs + PRODUCT_HEADERS,
                  lambda tmp: [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread"] + list(extra_flags) +
                  ["-o", str(tmp)] + [str(s) for s in srcs], force)
