"""Static checks on the gfx950 code object inside libaesw.so (CPU test: hipcc cross-compiles, llvm-objdump disassembles).

Why: the flush stores are `global_store_dwordx4 ... sc1` issued through inline asm (csrc/aesw_kernels.hip gstore /
gstore_at).  hipcc neither counts nor pads an inline-asm store, so the "VMEM store with more than 64 bits of data, then
a write of its data VGPRs" hazard is covered by a hand-placed `s_nop 1` inside the same asm statement.  Without it the
2^20-block test (and only that one) produced wrong bytes -- a silent-corruption class whose only guard used
to be a dynamic stress test.  This lint asserts, for every kernel in the library:
  * every `global_store_dwordx4 ... sc1` and every store in the SGPR-base form `global_store_dwordx4 v, v[..], s[..]` (the
    form gstore_at emits for all three flavours) is IMMEDIATELY followed by `s_nop >= 1`, every such dwordx2 store by an
    `s_nop` (the compiler emits neither sc1 nor SGPR-base stores by itself in this library: these are the inline-asm ones);
  * no scratch (`.private_segment_fixed_size == 0`), no VGPR spills, `.vgpr_count <= 256` (8 waves per CU);
and it compares every kernel's register / LDS / spill / store-instruction counts with the tracked table
`profiles/isa_resources.json`, so that a silent jump (104 -> 201 VGPRs happened once between two commits) shows up as a
diff a reviewer sees.  Regenerate the table on purpose with  AESW_UPDATE_ISA_JSON=1 python -m pytest tests/test_isa_lint.py
"""
import json
import re
from pathlib import Path

import pytest

from check_library import assert_tracked, resource_table
from isa_extract import extract, needs_llvm, short

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "profiles" / "isa_resources.json"


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    """The gfx950 code object of the built library, its disassembly and its kernel metadata."""
    return extract(ROOT / "halo2-aes_amd" / "libaesw.so", tmp_path_factory.mktemp("isa"))


def _short(demangled):
    """aesw::encrypt_kernel<1, true, 0, true, 2>(aesw::EncParams) -> encrypt_kernel<1,true,0,true,2>"""
    return short(demangled, drop="aesw::")


@needs_llvm
def test_every_inline_asm_store_is_padded(code_object):
    bad, n4, n2 = [], 0, 0
    for name, ins in code_object["funcs"].items():
        if name not in code_object["meta"]:
            continue
        if _short(code_object["demangled"][name]).startswith("check_kernel<"):
            continue  # no inline-asm store in it: its one store (the report's unit counts, a uniform pointer) is the compiler's own, hazards included
        for i, text in enumerate(ins):
            # inline-asm stores: every sc1 store, and every store in the SGPR-base form (gstore_at emits all three flavours so)
            m = re.match(r"^global_store_dwordx([24])\b.*(\bsc1\b|, s\[\d+:\d+\])", text)
            if not m:
                continue
            wide = m.group(1) == "4"
            n4 += wide
            n2 += not wide
            nxt = ins[i + 1] if i + 1 < len(ins) else ""
            mn = re.match(r"^s_nop (\d+)$", nxt)
            if not mn or (wide and int(mn.group(1)) < 1):
                bad.append("%s: instruction %d `%s` is followed by `%s`" % (code_object["demangled"][name], i, text, nxt))
    assert n4 > 1000, "the sc1 stores of the witness kernels were not found: has the store flavour changed? (%d, %d)" % (n4, n2)
    assert not bad, "\n".join(bad[:20])


@needs_llvm
def test_no_scratch_no_vgpr_spills_and_the_tracked_resource_table(code_object):
    table = resource_table(code_object, {
        "stores_x4_sc1": lambda t: bool(re.match(r"^global_store_dwordx4\b.*\bsc1\b", t)),
        "stores_x4_other": lambda t: bool(re.match(r"^global_store_dwordx4\b", t)) and " sc1" not in t,
        "ds_read_b128": "ds_read_b128",
        "v_perm_b32": "v_perm_b32",
        "readlane_writelane": ("v_readlane_b32", "v_writelane_b32"),
    }, drop="aesw::", max_unified=None)
    assert any(k.startswith("encrypt_kernel<1,true,0,true,2>") for k in table), sorted(table)[:5]
    # 256 unified registers = two waves per SIMD, what the 7 one-wave groups (packed) / two 3-wave groups per CU need.
    # The DENSE instantiations (a demoted option: 35 % of what they write are zeros) are allowed the whole file: they
    # run one wave per SIMD (two 2-wave groups per CU) and are launch-bounded accordingly in the source.
    over = [(k, row["vgpr"]) for k, row in table.items()
            if row["vgpr"] > (512 if k.startswith(("encrypt_kernel<0,", "key_kernel<0,")) else 256)]
    assert not over, "more unified registers than the launch geometry allows: %r" % over
    assert_tracked(table, TABLE)


@needs_llvm
def test_headline_kernel_shape(code_object):
    """The instantiation bench.py's headline launches: a hand-written CDNA4 kernel, not a byte loop."""
    table = json.loads(TABLE.read_text())
    k = table["encrypt_kernel<1,true,0,true,1>"]  # packed, xtime path, per-block keys + key witness, nontemporal stores
    assert k["stores_x4_other"] >= 100 and k["stores_x4_sc1"] == 0 and k["ds_read_b128"] >= 100 and k["v_perm_b32"] >= 300
    assert k["vgpr"] <= 256 and k["static_lds"] == 0
    # the three store flavours are the same code but for the cache-policy modifier (profiles/r03_study/README.md 2)
    for other in ("encrypt_kernel<1,true,0,true,0>", "encrypt_kernel<1,true,0,true,2>"):
        o = table[other]
        assert (o["vgpr"], o["sgpr_spill"]) == (k["vgpr"], k["sgpr_spill"]), other
        assert abs(o["instructions"] - k["instructions"]) <= k["instructions"] // 100, other  # the key-slab flush pads its sc1 stores itself
