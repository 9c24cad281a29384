"""Builds the product libraries in-tree.

  halo2-aes_amd/libaesw.so        HIP kernels + the C ABI of include/aesw.h (hipcc --offload-arch=gfx950)
  halo2-aes_amd/libaesw_host.so   the C++ mirror of the reference's host interface (include/aesw_host.h): plain g++,
                                  no device code, linked against libaesw.so -- it only calls the C ABI
  halo2-aes_amd/libaesw_<name>.so one library per entry of LIBRARIES, CURVE_LIBRARIES, PROOF_LIBRARIES, MULTIOPEN_LIBRARIES, VANISHING_LIBRARIES and BLINDING_LIBRARIES (the tables below say what each is; its public header is
                                  include/aesw_<name>.h): its own gfx950 kernels and entry points (hipcc), linked against
                                  libaesw.so, whose context it takes.  All are built by build_satellite() alike.

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
INCLUDE = ROOT / "include"


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


def _build(target: Path, deps, command, force: bool, in_place: bool = False) -> Path:
    """`target` from `deps`, unless it is newer than all of them and not forced.  `command(tmp)` is the argument list that writes
    the library to `tmp`.  Several ranks may get here at once (torchrun): serialise on a lock file, look again (another process
    may have built it while we waited), build under a private name, publish with an atomic rename.  in_place: the command
    names its own output (make), so `tmp` is the target itself."""
    if not force and _newer(target, deps):
        return target
    import fcntl
    with open(PKG / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and _newer(target, deps):
                return target
            tmp = target if in_place else target.with_suffix(".so.tmp%d" % os.getpid())
            _run(command(tmp))
            os.replace(tmp, target)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return target


def build_host(force: bool = False) -> Path:
    """libaesw_host.so: host code only (g++), NEEDED libaesw.so found next to it ($ORIGIN)."""
    host = PKG / "host"
    srcs = [host / "host_capi.cpp"]
    deps = srcs + [INCLUDE / "aesw.h", INCLUDE / "aesw_host.h", host / "halo2_lite.hpp", host / "aes_gadget.hpp", LIB]
    return _build(HOST_LIB, deps, lambda tmp: ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", str(tmp)] + [str(s) for s in srcs] +
                  ["-L" + str(PKG), "-laesw", "-Wl,-rpath,$ORIGIN"], force)


# The one list of what libaesw.so is made of: tools that build a private variant of the library (tools/trace.py, parts.py,
# key_ab.py, sanitize.sh) take it from here.
PRODUCT_SOURCES = [CSRC / n for n in ("aesw_kernels.hip", "aesw_api.cpp", "aesw_keyring.cpp", "aesw_hostpath.cpp", "aesw_arena.cpp",
                                      "aesw_comm.cpp", "aesw_group.cpp", "aesw_circuits.cpp")]
PRODUCT_HEADERS = [CSRC / n for n in ("aesw_lane.h", "aesw_layout.h", "aesw_flush.h", "aesw_slabmap.h", "aesw_check.h", "aesw_check_dev.h", "aesw_internal.h", "aesw_ctx.h",
                                      "aesw_keyring.h", "aesw_options.h", "aesw_placement.h", "aesw_align.h", "aesw_store.h", "aesw_report_dev.h", "aesw_fr.h", "aesw_mont.h")] + \
    [INCLUDE / "aesw.h"]


def _hipcc_shared(sources, out, extra_flags=(), link=()):
    """The one hipcc command line of a gfx950 shared library."""
    return [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread"] + list(extra_flags) + \
        ["-o", str(out)] + [str(s) for s in sources] + list(link)


def build_product(force: bool = False, extra_flags=(), out: Path = LIB, extra_sources=()) -> Path:
    """libaesw.so, or with `extra_flags` / `extra_sources` and another `out` a diagnostic variant of it (-DAESW_TRACE, ...)."""
    srcs = PRODUCT_SOURCES + [Path(s) for s in extra_sources]
    return _build(Path(out), srcs + PRODUCT_HEADERS, lambda tmp: _hipcc_shared(srcs, tmp, extra_flags), force)


# The thirteen libraries next to libaesw.so, in the order build() makes them (no dependency order: each needs libaesw.so alone).
# csrc/ itself holds exactly the sources of libaesw.so (PRODUCT_SOURCES); a library's live one level down, in csrc/<name>/.
# Each entry: its sources, the headers it depends on beyond SATELLITE_HEADERS, its public header.  SATELLITE_HEADERS is what
# every one of them may include: the context, the checker core, what an entry point says before it launches (aesw_entry.h;
# aesw_entry_rules.h, whose bounds are aesw_mult.h's), the store flavour (aesw_store.h), the report's reset and fold
# (aesw_report_dev.h), what a kernel of the libraries that compute in Fr does to a cell (aesw_fr_dev.h, over the aesw_fr.h each
# of them lists), the Montgomery arithmetic under every field (aesw_mont.h).  A new library is one more entry here (DESIGN 4.26 lists what else it brings).
#   circ   checks the witnesses of many circuits in one launch
#   cols   checks the assembled advice columns, as bytes or Fr cells
#   vals   checks a VALUES witness
#   acc    the lookup multiplicities of one circuit, accumulated chunk by chunk
#   perm   plookup's permuted columns, arranged from the multiplicities
#   vacc   the multiplicities accumulated from a VALUES witness
#   mult   the lookup multiplicities of a many-circuit batch
#   theta  the lookup arguments compressed under theta
#   grand  the grand product Z of every lookup argument, from beta and gamma
#   sigma  the grand products of the permutation argument, sigma as a column of cell indices
#   ntt    columns of Fr cells between Lagrange, coefficient and extended-coset form
#   quot   sigma as Fr columns, for the quotient h(X)
#   open   coefficient columns evaluated at points, folded under v and divided by (X - z)
SATELLITE_HEADERS = [CSRC / n for n in ("aesw_check_dev.h", "aesw_check.h", "aesw_layout.h", "aesw_slabmap.h", "aesw_internal.h", "aesw_ctx.h",
                                        "aesw_keyring.h", "aesw_options.h", "aesw_placement.h", "aesw_align.h", "aesw_entry.h", "aesw_entry_rules.h", "aesw_mult.h",
                                        "aesw_store.h", "aesw_report_dev.h", "aesw_fr_dev.h", "aesw_mont.h")] + [INCLUDE / "aesw.h", INCLUDE / "aesw_mult.h"]
LIBRARIES = {
    "circ": ([CSRC / "circ" / "aesw_circ_check.hip"], [CSRC / "aesw_circ_search.h"], INCLUDE / "aesw_circ.h"),
    "cols": ([CSRC / "cols" / "aesw_cols_check.hip"], [CSRC / "aesw_circ_search.h", CSRC / "aesw_fr.h"], INCLUDE / "aesw_cols.h"),
    "vals": ([CSRC / "vals" / "aesw_vals_check.hip"], [CSRC / "aesw_vals_check.h"], INCLUDE / "aesw_vals.h"),
    "acc": ([CSRC / "acc" / "aesw_acc.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h", CSRC / "aesw_run.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_acc.h"),
    "perm": ([CSRC / "perm" / "aesw_perm.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_perm.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_perm.h"),
    "vacc": ([CSRC / "vacc" / "aesw_vacc.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h", CSRC / "aesw_run.h", CSRC / "aesw_vals_check.h", CSRC / "aesw_vacc.h",
              INCLUDE / "aesw_mult.h"],
             INCLUDE / "aesw_vacc.h"),
    "mult": ([CSRC / "mult" / "aesw_mult.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h"], INCLUDE / "aesw_mult.h"),
    "theta": ([CSRC / "theta" / "aesw_theta.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_theta.h", CSRC / "aesw_mult.h", INCLUDE / "aesw_mult.h"],
              INCLUDE / "aesw_theta.h"),
    "grand": ([CSRC / "grand" / "aesw_grand.hip"],
              [CSRC / "aesw_fr.h", CSRC / "aesw_grand.h", CSRC / "aesw_theta.h", CSRC / "aesw_mult.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_grand.h"),
    "sigma": ([CSRC / "sigma" / "aesw_sigma.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h"], INCLUDE / "aesw_sigma.h"),
    "ntt": ([CSRC / "ntt" / "aesw_ntt.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h", CSRC / "aesw_ntt.h"], INCLUDE / "aesw_ntt.h"),
    "quot": ([CSRC / "quot" / "aesw_quot.hip"],
             [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h", CSRC / "aesw_ntt.h", CSRC / "aesw_theta.h", CSRC / "aesw_placement.h", CSRC / "aesw_quot.h"], INCLUDE / "aesw_quot.h"),
    "open": ([CSRC / "open" / "aesw_open.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_open.h"], INCLUDE / "aesw_open.h"),
}


def library_names() -> list:
    """Every library build_satellite() builds, in the order of LIBRARIES."""
    return list(LIBRARIES)


def library_entry(name: str):
    """(sources, headers beyond SATELLITE_HEADERS, public header) of `name`; KeyError if LIBRARIES has no such entry."""
    return LIBRARIES[name]


def _build_entry(name: str, entry, force: bool, extra_flags, out) -> Path:
    """libaesw_<name>.so from an entry of LIBRARIES, of CURVE_LIBRARIES, of PROOF_LIBRARIES, of MULTIOPEN_LIBRARIES, of VANISHING_LIBRARIES or of BLINDING_LIBRARIES: one hipcc line, NEEDED libaesw.so found next to it ($ORIGIN)."""
    sources, headers, public = entry
    return _build(PKG / (out or "libaesw_%s.so" % name), sources + SATELLITE_HEADERS + headers + [public, LIB],
                  lambda tmp: _hipcc_shared(sources, tmp, extra_flags, link=["-L" + str(PKG), "-laesw", "-Wl,-rpath,$ORIGIN"]), force)


def build_satellite(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of LIBRARIES: its kernels and its entry points (hipcc, gfx950), NEEDED libaesw.so found next to it ($ORIGIN).
    A library of its own: the kernel sets of libaesw.so and of the other satellites stay what they are.  With `extra_flags` and
    another `out` (a file name next to libaesw.so) a measurement variant of it (tools/vacc_bench.py: -DAESW_VACC_WAVES=16)."""
    return _build_entry(name, library_entry(name), force, extra_flags, out)


# The libraries that compute on the curve, built after LIBRARIES and in the same way (an entry has the same shape): a table of
# its own, because what they bring beyond Fr -- the base field aesw_fq.h, the group -- is theirs alone.
#   msm    columns of Fr cells or of bytes committed against a basis of points of bn256's G1
CURVE_LIBRARIES = {
    "msm": ([CSRC / "msm" / "aesw_msm.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_fq.h", CSRC / "aesw_msm.h"], INCLUDE / "aesw_msm.h"),
}


def curve_library_names() -> list:
    """Every library build_curve() builds, in the order of CURVE_LIBRARIES."""
    return list(CURVE_LIBRARIES)


def build_curve(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of CURVE_LIBRARIES, as build_satellite builds one of LIBRARIES.  With `extra_flags` and another
    `out` a measurement variant of it (tools/msm_bench.py: -DAESW_MSM_CHUNK=1024)."""
    return _build_entry(name, CURVE_LIBRARIES[name], force, extra_flags, out)


# The libraries that turn what the others computed into a proof, built after CURVE_LIBRARIES and in the same way (an entry has the
# same shape): a table of its own, because the first two are pinned at what they hold.
#   transcript  the Blake2b transcript: commitments and scalars absorbed, challenges squeezed, proof bytes written
PROOF_LIBRARIES = {
    "transcript": ([CSRC / "transcript" / "aesw_transcript.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_fq.h", CSRC / "aesw_transcript.h"], INCLUDE / "aesw_transcript.h"),
}


def proof_library_names() -> list:
    """Every library build_proof() builds, in the order of PROOF_LIBRARIES."""
    return list(PROOF_LIBRARIES)


def build_proof(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of PROOF_LIBRARIES, as build_satellite builds one of LIBRARIES."""
    return _build_entry(name, PROOF_LIBRARIES[name], force, extra_flags, out)


# The libraries of the multi-opening argument, built after PROOF_LIBRARIES and in the same way (an entry has the same shape): a
# table of its own, because the first three are pinned at what they hold.  (Not OPENING_LIBRARIES: tests/test_build_table.py holds
# that name gone, with the six tables that became LIBRARIES.)
#   shplonk  SHPLONK's two quotients h and W over every queried column: the sets' scalars, the combine, the quotient of a set
MULTIOPEN_LIBRARIES = {
    "shplonk": ([CSRC / "shplonk" / "aesw_shplonk.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_open.h", CSRC / "aesw_shplonk.h"], INCLUDE / "aesw_shplonk.h"),
}


def multiopen_library_names() -> list:
    """Every library build_multiopen() builds, in the order of MULTIOPEN_LIBRARIES."""
    return list(MULTIOPEN_LIBRARIES)


def build_multiopen(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of MULTIOPEN_LIBRARIES, as build_satellite builds one of LIBRARIES."""
    return _build_entry(name, MULTIOPEN_LIBRARIES[name], force, extra_flags, out)


# The libraries of the vanishing argument, built after MULTIOPEN_LIBRARIES and in the same way (an entry has the same shape): a
# table of its own, because the first four are pinned at what they hold.  (Not QUOTIENT_LIBRARIES: tests/test_build_table.py holds
# that name gone, with the six tables that became LIBRARIES.)
#   vanish  the quotient h(X) on the extended coset, folded one constraint segment per call
VANISHING_LIBRARIES = {
    "vanish": ([CSRC / "vanish" / "aesw_vanish.hip"],
               [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h", CSRC / "aesw_ntt.h", CSRC / "aesw_theta.h", CSRC / "aesw_quot.h", CSRC / "aesw_vanish.h"], INCLUDE / "aesw_vanish.h"),
}


def vanishing_library_names() -> list:
    """Every library build_vanishing() builds, in the order of VANISHING_LIBRARIES."""
    return list(VANISHING_LIBRARIES)


def build_vanishing(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of VANISHING_LIBRARIES, as build_satellite builds one of LIBRARIES."""
    return _build_entry(name, VANISHING_LIBRARIES[name], force, extra_flags, out)


# The libraries that blind, built after VANISHING_LIBRARIES and in the same way (an entry has the same shape): a table of its own,
# because the first five are pinned at what they hold.
#   blind  the blinding rows of a column from a seed in device memory, and the commitment of a column of bytes with a blinded tail
BLINDING_LIBRARIES = {
    "blind": ([CSRC / "blind" / "aesw_blind.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_fq.h", CSRC / "aesw_msm.h", CSRC / "aesw_transcript.h", CSRC / "aesw_blind.h"],
              INCLUDE / "aesw_blind.h"),
}


def blinding_library_names() -> list:
    """Every library build_blinding() builds, in the order of BLINDING_LIBRARIES."""
    return list(BLINDING_LIBRARIES)


def build_blinding(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of BLINDING_LIBRARIES, as build_satellite builds one of LIBRARIES."""
    return _build_entry(name, BLINDING_LIBRARIES[name], force, extra_flags, out)
