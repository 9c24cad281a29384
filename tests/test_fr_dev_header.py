"""The device core of the libraries that compute in Fr (csrc/aesw_fr_dev.h), read as text, without a GPU: the
header is there and every library may include it, each of the five libraries includes it and defines none of its helpers -- nor
an unroll -- itself, aesw_grand.h has handed its unroll to aesw_fr.h, and the header declares no kernel."""
import importlib.util
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "halo2-aes_amd" / "csrc"
HEADER = CSRC / "aesw_fr_dev.h"
LIBRARIES = ("theta", "grand", "sigma", "ntt", "quot")
SHARED = ("load_cell", "store_cell", "cell_at", r"shfl_\w+_cell", r"wave_scan\w*", "each", "unrolled", r"\w+_each", r"\w+_unrolled")


def _defined(text, name):
    """the definitions of a function `name` (a regular expression) in `text`: a return type, the name, a parameter list, a body"""
    return re.findall(r"^[^\n;=]*[\w>&*]\s+\*?(%s)\s*\([^;{]*\)\s*\{" % name, text, re.M)


def test_the_header_is_there_and_every_library_may_include_it():
    spec = importlib.util.spec_from_file_location("b", ROOT / "halo2-aes_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert HEADER.exists() and HEADER in b.SATELLITE_HEADERS
    text = HEADER.read_text()
    assert "__global__ void" not in text and not re.search(r"^\s*__global__", text, re.M)  # a kernel here would be one of every library
    for include in ('"aesw_fr.h"', '"aesw_store.h"', '"aesw_report_dev.h"'):
        assert "#include " + include in text, include
    assert "namespace aesw {" in text
    for name in ("load_cell", "store_cell", "cell_at", "shfl_up_cell", "shfl_down_cell", "shfl_xor_cell", "wave_scan_up", "wave_scan_down"):
        found = _defined(text, name)
        assert found, name
    # every function of it is device code, inlined where it is used
    assert len(re.findall(r"^(?:template[^\n]*\n)?__device__ __forceinline__ ", text, re.M)) == len(_defined(text, r"\w+"))


def test_the_finder_finds_a_private_copy():
    private = "namespace x {\n__device__ __forceinline__ Fr load_cell(const u32x4 *p) {\n    return Fr{};\n}\ntemplate <int N, class F>\n" \
              "__device__ __forceinline__ void unrolled(F &&f) {\n}\n__device__ __forceinline__ u32x4 *cell_at(u32x4 *base, uint64_t i) { return base + i * 2; }\n}"
    assert _defined(private, "load_cell") == ["load_cell"] and _defined(private, "unrolled") == ["unrolled"] and _defined(private, "cell_at") == ["cell_at"]
    assert not _defined("    if (at < cells) store_cell<0>(cell_at(out, at), v);\n    t = wave_scan_up(t, lane);\n", r"cell_at|wave_scan\w*")


def test_the_five_libraries_include_it_and_define_none_of_it_themselves():
    for name in LIBRARIES:
        text = (CSRC / name / ("aesw_%s.hip" % name)).read_text()
        assert '#include "../aesw_fr_dev.h"' in text, name
        for helper in SHARED:
            assert not _defined(text, helper), (name, helper)


def test_the_unroll_is_the_field_headers():
    assert _defined((CSRC / "aesw_fr.h").read_text(), "fr_unrolled") == ["fr_unrolled"]
    grand = (CSRC / "aesw_grand.h").read_text()
    assert "grand_unrolled" not in grand and "grand_each" not in grand and "fr_unrolled<" in grand
