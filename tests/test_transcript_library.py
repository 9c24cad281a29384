"""libaesw_transcript.so without a GPU: that build() makes it and what it is made of.

  * it exists after build(), exports exactly the aesw_transcript_ functions include/aesw_transcript.h declares,
    api.TRANSCRIPT_SYMBOLS binds exactly those, its NEEDED entry is libaesw.so via $ORIGIN and no other library of the project is one;
  * it is the entry of the third build table, _build.PROOF_LIBRARIES, and of api._PROOF_LIBRARIES -- not of the first two, which
    stay what their tests pin -- and build() builds it through build_proof and loads it;
  * a Group refuses; a missing path says how to build it;
  * every __global__ in it is launched by the GPU tests (tests/transcript_cases.py), and that list names nothing else;
  * its code object: no scratch, no VGPR spills, no atomic of any kind, global or LDS; the squeeze kernel holds the two field
    products of fr_from_u512 as 64-bit multiply-adds; one wave a workgroup, so at most 512 registers a lane, and the LDS of the
    absorb kernels does not grow with n (it is static); compared with the tracked table profiles/isa_resources_transcript.json
    (regenerate it on purpose with AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_transcript_library.py);
  * the other libraries carry none of the new symbols, and the header names no other library."""
import subprocess

import check_library as cl
import transcript_cases as tc
from isa_extract import needs_llvm

TABLE = cl.ROOT / "profiles" / "isa_resources_transcript.json"
code_object = cl.code_object_fixture("TRANSCRIPT_LIB_PATH")
DECLARED = ["aesw_transcript_chunk_points", "aesw_transcript_chunk_scalars", "aesw_transcript_init_device", "aesw_transcript_points_device", "aesw_transcript_scalars_device",
            "aesw_transcript_squeeze_device"]
METHODS = ("transcript",)
MAX_UNIFIED = 512  # one wave a workgroup: a lane may hold the whole file of its SIMD


def test_build_makes_the_library_and_it_exports_the_header(pkg):
    api = pkg.api
    lib = api.TRANSCRIPT_LIB_PATH
    assert lib.name == "libaesw_transcript.so" and lib.parent == api.LIB_PATH.parent and lib.exists()
    assert cl.declared("aesw_transcript.h", "aesw_transcript_") == DECLARED
    exported = {line.split()[-1] for line in cl.nm(lib, "-D", "--defined-only").splitlines() if " T " in line}
    assert sorted(f for f in exported if f.startswith("aesw_")) == DECLARED, sorted(exported)[:20]
    loaded = api.load_transcript_library()
    assert api.load_transcript_library() is loaded and sorted(api.TRANSCRIPT_SYMBOLS) == DECLARED and all(getattr(loaded, f) is not None for f in DECLARED)
    dyn = subprocess.run(["readelf", "-d", str(lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libaesw.so" in dyn and "$ORIGIN" in dyn, dyn
    b = cl.build_module()
    assert not [n for n in b.library_names() + b.curve_library_names() + ["host"] if "libaesw_%s" % n in dyn], dyn
    source = (cl.ROOT / "halo2-aes_amd" / "csrc" / "transcript" / "aesw_transcript.hip").read_text()
    assert "namespace aesw_transcript {" in source and '#include "../aesw_transcript.h"' in source
    header = (cl.ROOT / "include" / "aesw_transcript.h").read_text()
    assert '#include "aesw.h"' in header and header.count("#include \"aesw") == 1 and "#define AESW_TRANSCRIPT_STATE_BYTES 256u" in header
    assert not [n for n in b.library_names() + b.curve_library_names() if "aesw_" + n in header]


def test_the_third_table_has_the_shape_of_the_first_and_build_walks_it(pkg, monkeypatch):
    import __graft_entry__ as ge
    b, api = cl.build_module(), pkg.api
    assert b.proof_library_names() == ["transcript"] == list(b.PROOF_LIBRARIES) == list(api._PROOF_LIBRARIES)
    assert "transcript" not in b.LIBRARIES and "transcript" not in b.CURVE_LIBRARIES and "transcript" not in api._LIBRARIES and "transcript" not in api._CURVE_LIBRARIES
    assert len(b.LIBRARIES) == 13 and len(api._LIBRARIES) == 15 and list(b.CURVE_LIBRARIES) == ["msm"] == list(api._CURVE_LIBRARIES)
    sources, headers, public = b.PROOF_LIBRARIES["transcript"]
    assert sources and all(s.exists() and s.parent == b.CSRC / "transcript" and s.suffix == ".hip" for s in sources)
    assert [h.name for h in headers] == ["aesw_fr.h", "aesw_fq.h", "aesw_transcript.h"] and all(h.exists() and h.parent == b.CSRC for h in headers)
    assert public == b.INCLUDE / "aesw_transcript.h" and public.exists()
    assert api._PROOF_LIBRARIES["transcript"] == (api.TRANSCRIPT_LIB_PATH, api.TRANSCRIPT_SYMBOLS, api._NO_FALLBACK)
    built, loaded = [], []
    monkeypatch.setattr(b, "build_satellite", lambda name, force=False: built.append(name))
    monkeypatch.setattr(b, "build_curve", lambda name, force=False: built.append("curve:" + name))
    monkeypatch.setattr(b, "build_proof", lambda name, force=False: built.append("proof:" + name))
    monkeypatch.setattr(ge, "_load_build", lambda: b)
    monkeypatch.setattr(api, "load_transcript_library", lambda path=None: loaded.append("transcript"))
    ge.build()
    assert built == b.library_names() + ["curve:msm", "proof:transcript"] and loaded == ["transcript"]


def test_a_missing_path_says_how_to_build_it(pkg, tmp_path):
    cl.check_missing_path(pkg, "transcript", tmp_path)


def test_the_other_libraries_are_left_alone(pkg):
    others = dict(pkg.api._LIBRARIES, **pkg.api._CURVE_LIBRARIES)
    for other, (path, _symbols, _hint) in others.items():
        text = cl.nm(path, "-C")
        assert not [w for w in ("aesw_transcript", "transcript_init_kernel", "transcript_absorb_kernel", "transcript_squeeze_kernel") if w in text], other
    naming = sorted(h.name for h in (cl.ROOT / "include").glob("*.h") if h.name != "aesw_transcript.h" and "aesw_transcript" in h.read_text())
    assert naming == []


def test_a_group_refuses(pkg):
    cl.check_group_refuses(pkg, METHODS)


def test_every_kernel_of_the_library_is_launched_and_the_list_names_nothing_else(pkg):
    cl.check_swept(pkg.api.TRANSCRIPT_LIB_PATH, tc.launched())
    src = (cl.ROOT / "tests" / "test_gpu_transcript_stream.py").read_text()
    assert all(w in src for w in ("tc.cases(", "write_points", "write_scalars", "common_points", "common_scalars", "squeeze(", "aesw_transcript_chunk_points"))


@needs_llvm
def test_gfx950_code_without_scratch_spills_or_atomics_and_the_tracked_table(code_object):
    columns = dict(cl.GLOBAL_COLUMNS, lds_ops=lambda t: t.startswith("ds_"), barriers="s_barrier", mad_u64=lambda t: t.startswith("v_mad_u64_u32"),
                   atomics=lambda t: "atomic" in t or t.startswith(("ds_add", "ds_sub", "ds_inc", "ds_dec", "ds_min", "ds_max", "ds_and", "ds_or", "ds_xor", "ds_cmpst", "ds_wrxchg")))
    table = cl.resource_table(code_object, columns, max_unified=None)  # no scratch, no VGPR spills; the register bound is stated here
    assert set(table) == tc.launched(), sorted(table)
    for name, row in table.items():
        assert row["vgpr"] + row["agpr"] <= MAX_UNIFIED and row["sgpr_spill"] == 0, (name, row)
        assert row["atomics"] == 0 and row["global_atomics"] == 0, (name, row)
        if "squeeze" in name:  # a half of fr_from_u512 a lane: a product is 2 x 8 x 8 limb products; the state and the digest in LDS
            assert row["mad_u64"] >= 2 * 64 and row["static_lds"] == 256 + 64, (name, row)
        if "absorb" in name:  # a product by the raw 1: the reduction's 64 stay; the state, the stream of one chunk and its proof bytes
            assert row["mad_u64"] >= 64 and 256 + 128 + 64 * 33 <= row["static_lds"] <= 8192, (name, row)
        assert row["barriers"] == 0, (name, row)  # a workgroup is one wave: hipcc drops the barrier of __syncthreads and keeps its waits
        if "init" in name:
            assert row["static_lds"] == 0 and row["global_loads"] == 0, (name, row)
    cl.assert_tracked(table, TABLE)
