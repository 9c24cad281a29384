"""libaesw_blind.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_blind_ functions include/aesw_blind.h declares, api.BLIND_SYMBOLS binds exactly
    those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * it is the entry of the sixth build table, _build.BLINDING_LIBRARIES, and of api._BLINDING_LIBRARIES -- not of the first five,
    which stay what their tests pin -- and build() builds it through build_blinding, last, and loads it; _load consults the sixth
    table after the others;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/blind_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic of any kind, no LDS; the fill kernels hold the two field products of the
    wide reduction as 64-bit multiply-adds and store one cell a lane; the tail-commit kernel is one wave a workgroup, so at most 512
    registers a lane, stores 64 bytes, and its product loops stay rolled (its instruction count is far below what 254 unrolled
    steps would take); compared with the tracked table profiles/isa_resources_blind.json (regenerate it on purpose with
    AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_blind_library.py);
  * the other libraries carry none of the new symbols, and the header names no other library."""
import subprocess

import blind_cases as bc
import check_library as cl
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_blind.json"
code_object = cl.code_object_fixture("BLIND_LIB_PATH")
DECLARED = ["aesw_blind_commit_tail_device", "aesw_blind_max_tail", "aesw_blind_rows_device", "aesw_blind_tail_device", "aesw_blind_tail_rows"]
METHODS = ("blinding_seed", "blind_rows", "blinding_tail", "commit_tail", "commit_blinded_bytes")
MAX_UNIFIED = 512  # one wave a workgroup: a lane may hold the whole file of its SIMD


def other_tables(b, api):
    return (b.LIBRARIES, b.CURVE_LIBRARIES, b.PROOF_LIBRARIES, b.MULTIOPEN_LIBRARIES, b.VANISHING_LIBRARIES,
            api._LIBRARIES, api._CURVE_LIBRARIES, api._PROOF_LIBRARIES, api._MULTIOPEN_LIBRARIES, api._VANISHING_LIBRARIES)


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.BLIND_LIB_PATH
    assert lib.name == "libaesw_blind.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    assert cl.declared("aesw_blind.h", "aesw_blind_") == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == DECLARED, sorted(exported)[:20]
    loaded = api.load_blind_library()
    assert api.load_blind_library() is loaded and sorted(api.BLIND_SYMBOLS) == DECLARED and all(getattr(loaded, f) is not None for f in DECLARED)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = cl.build_module()
    others = b.library_names() + b.curve_library_names() + b.proof_library_names() + b.multiopen_library_names() + b.vanishing_library_names()
    assert not [n for n in others + ["host"] if "libaesw_%s" % n in dyn], dyn
    source = (cl.ROOT / "halo2-aes_amd" / "csrc" / "blind" / "aesw_blind.hip").read_text()
    assert "namespace aesw_blind {" in source and all('#include "../%s"' % h in source for h in ("aesw_fr_dev.h", "aesw_blind.h", "aesw_entry.h"))
    header = (cl.ROOT / "include" / "aesw_blind.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1
    assert "#define AESW_BLIND_MAX_TAIL %du" % int(loaded.aesw_blind_max_tail()) in header and "#define AESW_BLIND_SEED_BYTES %du" % api.BLIND_SEED_BYTES in header
    assert not [n for n in others if "aesw_" + n in header]


def test_the_sixth_table_has_the_shape_of_the_first_and_build_walks_it_last(pkg, monkeypatch):
    import __graft_entry__ as ge
    b, api = cl.build_module(), pkg.api
    assert b.blinding_library_names() == ["blind"] == list(b.BLINDING_LIBRARIES) == list(api._BLINDING_LIBRARIES)
    assert not [t for t in other_tables(b, api) if "blind" in t]
    # the first five tables stay what their tests pin
    assert len(b.LIBRARIES) == 13 and len(api._LIBRARIES) == 15 and list(b.CURVE_LIBRARIES) == ["msm"] == list(api._CURVE_LIBRARIES)
    assert list(b.PROOF_LIBRARIES) == ["transcript"] == list(api._PROOF_LIBRARIES) and list(b.MULTIOPEN_LIBRARIES) == ["shplonk"] == list(api._MULTIOPEN_LIBRARIES)
    assert list(b.VANISHING_LIBRARIES) == ["vanish"] == list(api._VANISHING_LIBRARIES)
    sources, headers, public = b.BLINDING_LIBRARIES["blind"]
    assert sources and all(s.exists() and s.parent == b.CSRC / "blind" and s.suffix == ".hip" for s in sources)
    assert [h.name for h in headers] == ["aesw_fr.h", "aesw_fq.h", "aesw_msm.h", "aesw_transcript.h", "aesw_blind.h"]
    assert all(h.exists() and h.parent == b.CSRC for h in headers)
    assert public == b.INCLUDE / "aesw_blind.h" and public.exists()
    assert api._BLINDING_LIBRARIES["blind"] == (api.BLIND_LIB_PATH, api.BLIND_SYMBOLS, api._NO_FALLBACK)
    built, loaded = [], []
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    for table in ("curve", "proof", "multiopen", "vanishing", "blinding"):
        monkeypatch.setattr(b, "build_" + table, lambda name, force=False, table=table: built.append(table + ":" + name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    for name in ("vanish", "blind"):
        monkeypatch.setattr(api, "load_%s_library" % name, lambda path=None, name=name: loaded.append(name))
    ge.build()
    assert built == b.library_names() + ["curve:msm", "proof:transcript", "multiopen:shplonk", "vanishing:vanish", "blinding:blind"] and loaded == ["vanish", "blind"]


def test_the_loader_consults_the_sixth_table_after_the_others(pkg, monkeypatch):
    api = pkg.api
    # a name of an earlier table wins over the same name in the sixth: the order of _load's tables
    decoy = (api.BLIND_LIB_PATH.with_name("libaesw_nowhere.so"), {}, "")
    monkeypatch.setitem(api._BLINDING_LIBRARIES, "msm", decoy)
    monkeypatch.setattr(api, "_loaded", {})
    assert api._load("msm", None)._name == str(api.MSM_LIB_PATH)
    assert api._load("blind", None)._name == str(api.BLIND_LIB_PATH)


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "blind", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    api = pkg.api
    others = dict(api._LIBRARIES, **api._CURVE_LIBRARIES, **api._PROOF_LIBRARIES, **api._MULTIOPEN_LIBRARIES, **api._VANISHING_LIBRARIES)
    for other, (path, _symbols, _hint) in others.items():
        text = cl.nm(path, "-C")
        assert not [w for w in ("aesw_blind", "blind_cells_kernel", "blind_commit_tail_kernel") if w in text], other
    naming = sorted(h.name for h in (cl.ROOT / "include").glob("*.h") if h.name != "aesw_blind.h" and "aesw_blind" in h.read_text())
    assert naming == []


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_the_python_face_refuses_a_size_before_it_sizes_anything(pkg):
    """_blind_tail and blinding_seed need no device"""
    api = pkg.api
    ctx = api.Context.__new__(api.Context)
    for args in ((9, 1, 0), (29, 1, 0), (10, 0, 1018), (10, 65536, 1018), (10, 1, 1024), (10, 1, -1), (10, 1, 0, 1 << 64), (10, 1, 0, 0, -1)):
        try:
            ctx._blind_tail("aesw_blind_rows_device", *args)
        except pkg.AeswError as e:
            assert e.status == api.ERR_INVALID_ARG and "aesw_blind_rows_device" in str(e)
        else:
            raise AssertionError(args)
    assert ctx._blind_tail("call", 10, 3, 1018, bc.BIG_DOMAIN, 1 << 40)[1:] == (10, 3, 1018, bc.BIG_DOMAIN, 1 << 40, 6)
    try:
        ctx.blinding_seed(b"short")
    except ValueError:
        pass
    else:
        raise AssertionError("a seed of five bytes")


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.BLIND_LIB_PATH, bc.launched())
    assert len(bc.launched()) == 4
    for name, words in (("test_gpu_blind_cells.py", ("bc.STORE_MODES", "bc.FILL_TAILS", "blind_rows", "blinding_tail", "fr_store_mode")),
                        ("test_gpu_blind_commit.py", ("bc.COMMIT_TAILS", "commit_tail", "commit_blinded_bytes", "aesw_msm_chunk_rows")),
                        ("test_gpu_blind_calls.py", ("aesw_blind_%s_device", "torch.cuda.graph", "examples"))):
        src = (cl.ROOT / "tests" / name).read_text()
        assert all(w in src for w in words), name


@needs_llvm
def test_gfx950_code_without_scratch_spills_lds_or_atomics_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_") and not t.startswith(("ds_bpermute", "ds_swizzle", "ds_permute")), barriers="s_barrier",
                   mad_u64=lambda t: t.startswith("v_mad_u64_u32"), atomics=lambda t: "atomic" in t)
    table = cl.resource_table(code_object, columns, max_unified=None)  # no scratch, no VGPR spills; the register bound is stated here
    assert set(table) == bc.launched(), sorted(table)
    for name, row in table.items():
        assert row["sgpr_spill"] == 0 and row["atomics"] == 0 and row["global_atomics"] == 0, (name, row)
        assert row["static_lds"] == 0 and row["lds_ops"] == 0 and row["barriers"] == 0, (name, row)
        if "cells" in name:  # two products of the wide reduction: 2 x 8 x 8 limb products each; one cell a lane, two 16-byte pieces
            assert row["vgpr"] + row["agpr"] <= 256 and row["mad_u64"] >= 2 * 2 * 64 and row["global_stores"] == 2, (name, row)
        else:  # one wave: up to 512 registers; 64 bytes stored; the loops that hold the products stay loops
            assert row["vgpr"] + row["agpr"] <= MAX_UNIFIED and row["global_stores"] == 4, (name, row)
            # a doubling and a mixed addition are 19 products of 128 multiply-adds: 254 unrolled steps would be over 600 000 of them
            assert row["mad_u64"] >= 64 and row["mad_u64"] < 128 * 19 * 16 and row["instructions"] < 200000, (name, row)
    cl.assert_tracked(table, TABLE)
