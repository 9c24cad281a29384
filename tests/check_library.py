"""What the CPU tests of the built libraries share (the thirteen test_*_library.py, test_build_table.py, test_library_loader.py,
test_circuits_coverage.py, test_isa_lint.py): the build table, the kernels and exports `nm` shows, the functions a public
header declares, what every library next to libaesw.so is held to (check_*), and the per-kernel resource table of a code object (isa_extract.py) held against its tracked JSON
under profiles/.  Regenerate a tracked table on purpose with  AESW_UPDATE_ISA_JSON=1 python -m pytest tests/<the test file>."""
import importlib.util
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

from isa_extract import extract, short

ROOT = Path(__file__).resolve().parent.parent

_ANY_STUB = re.compile(r"([\w:]*?)__device_stub__(\w+)(<[^()]*>)?\(")


def nm(path, *flags):
    return subprocess.run(["nm", *flags, str(path)], stdout=subprocess.PIPE, text=True, check=True).stdout


def all_kernels(nm_text):
    """(namespace, kernel name with template arguments, spaces removed) of every __global__ instantiation's host stub."""
    return {(m.group(1).rstrip(":"), m.group(2) + (m.group(3) or "").replace(" ", "")) for m in _ANY_STUB.finditer(nm_text)}


def declared(header, prefix):
    """The functions include/<header> declares whose names start with `prefix`, sorted."""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, text)))


_header_declares = declared  # check_exports takes the caller's list under that name


def build_module():
    """halo2-aes_amd/_build.py as a module of its own: the build table, without importing the package."""
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def check_exports(pkg, name, declared=None):
    """libaesw_<name>.so is where build() puts it, exports exactly the aesw_<name>_ functions include/aesw_<name>.h declares
    (`declared`, where the caller lists them) and no other aesw_ symbol, api.py binds exactly those and caches the default
    load, and its one NEEDED library of the project is libaesw.so (whose contexts it takes), found next to itself.  Returns
    the declared names."""
    api, prefix = pkg.api, "aesw_%s_" % name
    lib, symbols = getattr(api, name.upper() + "_LIB_PATH"), getattr(api, name.upper() + "_SYMBOLS")
    assert lib.name == "libaesw_%s.so" % name and lib.parent == api.LIB_PATH.parent and lib.exists()
    decl = _header_declares("aesw_%s.h" % name, prefix)
    assert declared is None or decl == declared
    exported = {line.split()[-1] for line in nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == decl, sorted(exported)[:20]
    load = getattr(api, "load_%s_library" % name)
    loaded = load()
    assert load() is loaded
    assert sorted(symbols) == decl and all(getattr(loaded, f) is not None for f in decl)
    assert api._LIBRARIES[name] == (lib, symbols, api._NO_FALLBACK)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = build_module()
    assert not [n for n in b.library_names() + ["host"] if "libaesw_%s" % n in dyn], dyn
    # the sources live one level below csrc/, which keeps holding exactly the sources of libaesw.so
    sources = b.library_entry(name)[0]
    assert sources and all(s.exists() and s.parent == ROOT / "halo2-aes_amd" / "csrc" / name for s in sources), sources
    return decl


def check_others_left_alone(pkg, name, words, named_by=(), symbol=None):
    """No other library of api._LIBRARIES carries `aesw_<name>` (`symbol`, where the caller narrows it) or one of `words` (its
    kernels) in `nm -C`, and the public headers that name `aesw_<name>` are its own and exactly `named_by`: the headers of the
    libraries built over it, which say so."""
    for other, (path, _symbols, _hint) in pkg.api._LIBRARIES.items():
        if other != name:
            text = nm(path, "-C")
            assert not [w for w in (symbol or "aesw_" + name,) + tuple(words) if w in text], other
    naming = sorted(h.name for h in (ROOT / "include").glob("*.h") if h.name != "aesw_%s.h" % name and "aesw_" + name in h.read_text())
    assert naming == sorted(named_by), naming


def check_missing_path(pkg, name, tmp_path):
    """A path that does not exist is a FileNotFoundError that names it and says that nothing stands in for the library."""
    missing = tmp_path / "nowhere" / getattr(pkg.api, name.upper() + "_LIB_PATH").name
    with pytest.raises(FileNotFoundError) as e:
        getattr(pkg.api, "load_%s_library" % name)(missing)
    assert str(missing) in str(e.value) and "There is no fallback implementation." in str(e.value)


def check_group_refuses(pkg, methods):
    """Each of `methods` exists on Context and is refused by a Group with ERR_INVALID_ARG."""
    for method in methods:
        assert callable(getattr(pkg.api.Context, method)), method
        with pytest.raises(pkg.AeswError) as e:
            getattr(pkg.Group, method)(None)
        assert e.value.status == pkg.api.ERR_INVALID_ARG


def check_swept(lib, launched):
    """Every __global__ instantiation in the library at `lib` is in `launched` (what a GPU sweep launches), and nothing else is."""
    kernels = {"%s::%s" % (ns, k) if ns else k for ns, k in all_kernels(nm(lib, "-C"))}
    assert kernels == launched, (sorted(kernels), sorted(launched))


def code_object_fixture(lib_path_name):
    """A module-scoped fixture: the gfx950 code object (isa_extract.extract) of the library api.<lib_path_name> names."""
    @pytest.fixture(scope="module")
    def code_object(pkg, tmp_path_factory):
        co = extract(getattr(pkg.api, lib_path_name), tmp_path_factory.mktemp("isa"))
        assert co["target"].endswith("gfx950"), co["target"]
        return co
    return code_object


GLOBAL_COLUMNS = {"global_loads": "global_load_", "global_stores": "global_store_", "global_atomics": "global_atomic_"}


def instructions(code_object, drop=""):
    """short kernel name (isa_extract.short) -> its instruction list"""
    return {short(code_object["demangled"][name], drop): code_object["funcs"].get(name, []) for name in code_object["meta"]}


def resource_table(code_object, extra_columns, drop="", max_unified=256):
    """short kernel name -> its row of the tracked table: registers, spills, static LDS, instruction count, then one count per
    entry of `extra_columns` (column -> an instruction prefix, or a predicate of the instruction text), in that order.  No kernel
    may use scratch or spill VGPRs, nor hold more than `max_unified` registers (256: two waves per SIMD; None: the caller's rule)."""
    table = {}
    for name, k in code_object["meta"].items():
        kernel, ins = short(code_object["demangled"][name], drop), code_object["funcs"].get(name, [])
        assert k[".private_segment_fixed_size"] == 0, "%s uses %d B of scratch" % (kernel, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0, "%s spills VGPRs" % kernel
        row = {"vgpr": k[".vgpr_count"], "agpr": k.get(".agpr_count", 0), "sgpr": k[".sgpr_count"],
               "sgpr_spill": k.get(".sgpr_spill_count", 0), "static_lds": k[".group_segment_fixed_size"], "instructions": len(ins)}
        assert max_unified is None or row["vgpr"] + row["agpr"] <= max_unified, (kernel, row)
        for column, what in extra_columns.items():
            row[column] = sum(1 for t in ins if (what(t) if callable(what) else t.startswith(what)))
        table[kernel] = row
    return dict(sorted(table.items()))


def assert_tracked(table, path):
    """`table` is what the tracked JSON at `path` holds; a difference is reported per kernel and column."""
    rel = path.relative_to(ROOT)
    if os.environ.get("AESW_UPDATE_ISA_JSON"):
        path.write_text(json.dumps(table, indent=1) + "\n")
    assert path.exists(), "%s is missing: run with AESW_UPDATE_ISA_JSON=1 and commit it" % rel
    tracked = json.loads(path.read_text())
    drift = []
    for name in sorted(set(table) | set(tracked)):
        a, b = tracked.get(name), table.get(name)
        if a and b and a != b:
            drift.append("%s: %s" % (name, ", ".join("%s %s -> %s" % (f, a.get(f), b.get(f)) for f in sorted(set(a) | set(b)) if a.get(f) != b.get(f))))
        elif a != b:
            drift.append("%s: only in the %s" % (name, "tracked table" if a else "built library"))
    assert not drift, ("the built kernels differ from %s (regenerate it with AESW_UPDATE_ISA_JSON=1 and commit the diff if the "
                       "change is intended):\n%s" % (rel, "\n".join(drift[:30])))
