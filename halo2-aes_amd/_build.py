"""Builds the product libraries in-tree.

  halo2-aes_amd/libaesw.so        HIP kernels + the C ABI of include/aesw.h (hipcc --offload-arch=gfx950)
  halo2-aes_amd/libaesw_host.so   the C++ mirror of the reference's host interface (include/aesw_host.h): plain g++,
                                  no device code, linked against libaesw.so -- it only calls the C ABI
  halo2-aes_amd/libaesw_<name>.so one library per entry of SATELLITES (the checkers -- circ: many circuits, include/aesw_circ.h;
                                  cols: the assembled advice columns, include/aesw_cols.h; vals: a VALUES witness,
                                  include/aesw_vals.h --, mult: the lookup multiplicities, include/aesw_mult.h, acc: the same
                                  accumulated chunk by chunk, include/aesw_acc.h, vacc: accumulated from a VALUES
                                  witness, include/aesw_vacc.h, and perm: plookup's permuted columns arranged from
                                  them, include/aesw_perm.h): its
                                  own gfx950 kernels and entry point (hipcc), linked against libaesw.so, whose context it
                                  takes.  All are built by build_satellite() alike.
  halo2-aes_amd/libaesw_theta.so  the one entry of FIELD_LIBRARIES: the lookup arguments compressed under theta
                                  (include/aesw_theta.h), built by build_satellite() as well
  halo2-aes_amd/libaesw_grand.so  the first entry of ARGUMENT_LIBRARIES: the grand product Z of every lookup argument from
                                  beta and gamma (include/aesw_grand.h), built by build_satellite() as well
  halo2-aes_amd/libaesw_sigma.so  the second entry of ARGUMENT_LIBRARIES: the grand products of the permutation argument from
                                  beta and gamma, sigma as a column of cell indices (include/aesw_sigma.h), built alike
  halo2-aes_amd/libaesw_ntt.so    the one entry of DOMAIN_LIBRARIES: columns of Fr cells between Lagrange, coefficient and
                                  extended-coset form (include/aesw_ntt.h), built alike
  halo2-aes_amd/libaesw_quot.so   the one entry of QUOTIENT_LIBRARIES: sigma as Fr columns, for the quotient h(X)
                                  (include/aesw_quot.h), built alike
  halo2-aes_amd/libaesw_open.so   the one entry of OPENING_LIBRARIES: coefficient columns evaluated at points, folded under v and
                                  divided by (X - z) (include/aesw_open.h), built alike

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
                                      "aesw_keyring.h", "aesw_options.h", "aesw_placement.h", "aesw_align.h", "aesw_store.h", "aesw_report_dev.h", "aesw_fr.h")] + \
    [INCLUDE / "aesw.h"]


def _hipcc_shared(sources, out, extra_flags=(), link=()):
    """The one hipcc command line of a gfx950 shared library."""
    return [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread"] + list(extra_flags) + \
        ["-o", str(out)] + [str(s) for s in sources] + list(link)


def build_product(force: bool = False, extra_flags=(), out: Path = LIB, extra_sources=()) -> Path:
    """libaesw.so, or with `extra_flags` / `extra_sources` and another `out` a diagnostic variant of it (-DAESW_TRACE, ...)."""
    srcs = PRODUCT_SOURCES + [Path(s) for s in extra_sources]
    return _build(Path(out), srcs + PRODUCT_HEADERS, lambda tmp: _hipcc_shared(srcs, tmp, extra_flags), force)


# The checker libraries next to libaesw.so.  csrc/ itself holds exactly the sources of libaesw.so (PRODUCT_SOURCES); a
# satellite's live one level down, in csrc/<name>/.  Each entry: its sources, the headers it depends on beyond
# SATELLITE_HEADERS, its public header.  SATELLITE_HEADERS is what every one of them may include: the context, the checker
# core, what an entry point says before it launches (aesw_entry.h; aesw_entry_rules.h, whose bounds are aesw_mult.h's), the
# store flavour (aesw_store.h), the report's reset and fold (aesw_report_dev.h), what a kernel of the libraries that compute
# in Fr does to a cell (aesw_fr_dev.h, over the aesw_fr.h each of them lists).  (The order is no build order -- each depends on libaesw.so alone -- but "mult" stays
# the last entry: tests/test_mult_library.py holds it there.)
SATELLITE_HEADERS = [CSRC / n for n in ("aesw_check_dev.h", "aesw_check.h", "aesw_layout.h", "aesw_slabmap.h", "aesw_internal.h", "aesw_ctx.h",
                                        "aesw_keyring.h", "aesw_options.h", "aesw_placement.h", "aesw_align.h", "aesw_entry.h", "aesw_entry_rules.h", "aesw_mult.h",
                                        "aesw_store.h", "aesw_report_dev.h", "aesw_fr_dev.h")] + [INCLUDE / "aesw.h", INCLUDE / "aesw_mult.h"]
SATELLITES = {
    "circ": ([CSRC / "circ" / "aesw_circ_check.hip"], [CSRC / "aesw_circ_search.h"], INCLUDE / "aesw_circ.h"),
    "cols": ([CSRC / "cols" / "aesw_cols_check.hip"], [CSRC / "aesw_circ_search.h", CSRC / "aesw_fr.h"], INCLUDE / "aesw_cols.h"),
    "vals": ([CSRC / "vals" / "aesw_vals_check.hip"], [CSRC / "aesw_vals_check.h"], INCLUDE / "aesw_vals.h"),
    "acc": ([CSRC / "acc" / "aesw_acc.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h", CSRC / "aesw_run.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_acc.h"),
    "perm": ([CSRC / "perm" / "aesw_perm.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_perm.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_perm.h"),
    "vacc": ([CSRC / "vacc" / "aesw_vacc.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h", CSRC / "aesw_run.h", CSRC / "aesw_vals_check.h", CSRC / "aesw_vacc.h",
              INCLUDE / "aesw_mult.h"],
             INCLUDE / "aesw_vacc.h"),
    "mult": ([CSRC / "mult" / "aesw_mult.hip"], [CSRC / "aesw_mult.h", CSRC / "aesw_mult_dev.h"], INCLUDE / "aesw_mult.h"),
}
CIRC_LIB, COLS_LIB, VALS_LIB, ACC_LIB, PERM_LIB, VACC_LIB, MULT_LIB = (PKG / ("libaesw_%s.so" % name) for name in SATELLITES)

# The libraries that do field arithmetic (csrc/aesw_fr.h), entries of the same shape.  A table of their own: SATELLITES is the
# seven libraries that move bytes and row indices and never touch Fr -- its length, its order and the tuple unpacked below it
# are held by the library tests of its entries.  This table is the compression under theta alone -- the test of its entry holds
# it at that -- and what needs the later challenges lives in ARGUMENT_LIBRARIES below.  build_satellite() looks a name up in
# all three tables (library_entry); __graft_entry__.build() walks library_names().
FIELD_LIBRARIES = {
    "theta": ([CSRC / "theta" / "aesw_theta.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_theta.h", CSRC / "aesw_mult.h", INCLUDE / "aesw_mult.h"],
              INCLUDE / "aesw_theta.h"),
}
THETA_LIB = PKG / "libaesw_theta.so"

# What needs beta and gamma: the libraries that build halo2's grand products once those challenges are known, entries of the
# same shape.  "grand" (the lookup arguments) shares the field header and the rules of theta (which table an argument reads, the
# row-order table index); "sigma" (the permutation argument) needs the field header and its own rules alone.
ARGUMENT_LIBRARIES = {
    "grand": ([CSRC / "grand" / "aesw_grand.hip"],
              [CSRC / "aesw_fr.h", CSRC / "aesw_grand.h", CSRC / "aesw_theta.h", CSRC / "aesw_mult.h", INCLUDE / "aesw_mult.h"], INCLUDE / "aesw_grand.h"),
    "sigma": ([CSRC / "sigma" / "aesw_sigma.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h"], INCLUDE / "aesw_sigma.h"),
}
GRAND_LIB = PKG / "libaesw_grand.so"
SIGMA_LIB = PKG / "libaesw_sigma.so"


# What changes the domain a column is given on: the number-theoretic transform.  It needs the field header, omega_k of the
# permutation argument's rules and its own rules.  A fourth table: the tests of the three above hold library_names() at what it is,
# so the entries of this one are named by domain_library_names() and __graft_entry__.build() walks them behind the others.
DOMAIN_LIBRARIES = {
    "ntt": ([CSRC / "ntt" / "aesw_ntt.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h", CSRC / "aesw_ntt.h"], INCLUDE / "aesw_ntt.h"),
}
NTT_LIB = PKG / "libaesw_ntt.so"


# What the quotient of the circuit's constraints needs: today sigma as Fr columns, with the rules of the fold.  It needs the field header and the rules of the
# permutation argument (the column order, delta), of the transforms (zeta, the table split) and of theta (the arity of a tag) next
# to its own.  A fifth table, named by quotient_library_names(): library_names() and domain_library_names() are held at what they
# are by the tests of the tables above, and __graft_entry__.build() walks this one last.
QUOTIENT_LIBRARIES = {
    "quot": ([CSRC / "quot" / "aesw_quot.hip"],
             [CSRC / "aesw_fr.h", CSRC / "aesw_sigma.h", CSRC / "aesw_ntt.h", CSRC / "aesw_theta.h", CSRC / "aesw_placement.h", CSRC / "aesw_quot.h"], INCLUDE / "aesw_quot.h"),
}
QUOT_LIB = PKG / "libaesw_quot.so"


# What the prover does with coefficient columns after its last challenge: evaluations at points, the fold under v and the division
# by (X - z).  It needs the field header and its own rules alone.  A sixth table, named by opening_library_names(): the three name
# functions above are held at what they are by the tests of the tables above, and __graft_entry__.build() walks this one last.
OPENING_LIBRARIES = {
    "open": ([CSRC / "open" / "aesw_open.hip"], [CSRC / "aesw_fr.h", CSRC / "aesw_open.h"], INCLUDE / "aesw_open.h"),
}
OPEN_LIB = PKG / "libaesw_open.so"


def library_names() -> list:
    """Every library build_satellite() builds, in the order of the three tables."""
    return list(SATELLITES) + list(FIELD_LIBRARIES) + list(ARGUMENT_LIBRARIES)


def domain_library_names() -> list:
    """The entries of DOMAIN_LIBRARIES: built by build_satellite() as well, behind library_names()."""
    return list(DOMAIN_LIBRARIES)


def quotient_library_names() -> list:
    """The entries of QUOTIENT_LIBRARIES: built by build_satellite() as well, behind domain_library_names()."""
    return list(QUOTIENT_LIBRARIES)


def opening_library_names() -> list:
    """The entries of OPENING_LIBRARIES: built by build_satellite() as well, behind quotient_library_names()."""
    return list(OPENING_LIBRARIES)


def library_entry(name: str):
    """(sources, headers beyond SATELLITE_HEADERS, public header) of `name`, whichever of the six tables holds it."""
    for table in (SATELLITES, FIELD_LIBRARIES, ARGUMENT_LIBRARIES, DOMAIN_LIBRARIES, QUOTIENT_LIBRARIES, OPENING_LIBRARIES):
        if name in table:
            return table[name]
    raise KeyError(name)


def build_satellite(name: str, force: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """libaesw_<name>.so of an entry of SATELLITES, FIELD_LIBRARIES, ARGUMENT_LIBRARIES, DOMAIN_LIBRARIES, QUOTIENT_LIBRARIES or OPENING_LIBRARIES: its kernels and its entry points (hipcc, gfx950), NEEDED libaesw.so found next to it ($ORIGIN).
    A library of its own: the kernel sets of libaesw.so and of the other satellites stay what they are.  With `extra_flags` and
    another `out` (a file name next to libaesw.so) a measurement variant of it (tools/vacc_bench.py: -DAESW_VACC_WAVES=16)."""
    sources, headers, public = library_entry(name)
    return _build(PKG / (out or "libaesw_%s.so" % name), sources + SATELLITE_HEADERS + headers + [public, LIB],
                  lambda tmp: _hipcc_shared(sources, tmp, extra_flags, link=["-L" + str(PKG), "-laesw", "-Wl,-rpath,$ORIGIN"]), force)
