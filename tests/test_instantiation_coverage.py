"""Every kernel instantiation in libaesw.so is launched by tests/test_gpu_instantiations.py (CPU: reads `nm -C` only).

The launched set is derived from tests/kernel_cases.py's case table through the dispatch rules restated there; adding a
template instantiation to the library without a sweep case fails here on any machine."""
import re
import subprocess

import kernel_cases as kc

_STUB = re.compile(r"aesw::__device_stub__(\w+)(<[^()]*>)?\(")


def library_kernels(nm_text):
    """Kernel names (template arguments without spaces) from `nm -C` output: one host stub per __global__ instantiation."""
    return {m.group(1) + (m.group(2) or "").replace(" ", "") for m in _STUB.finditer(nm_text)}


def _nm(pkg):
    return subprocess.run(["nm", "-C", str(pkg.api.LIB_PATH)], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_library_kernels_parse():
    text = ("000000000024d470 W void aesw::__device_stub__key_kernel<0, false, 0>(aesw::KeyParams)\n"
            "0000000000236960 T aesw::__device_stub__table_kernel(unsigned char const*, unsigned char*)\n"
            "000000000026f8e8 V void aesw::key_kernel<0, false, 0>(aesw::KeyParams)\n")
    assert library_kernels(text) == {"key_kernel<0,false,0>", "table_kernel"}


def test_every_instantiation_is_swept(pkg):
    lib = library_kernels(_nm(pkg))
    assert len(lib) >= 100, "too few kernels found in nm -C output: %r" % sorted(lib)[:5]
    swept = kc.launched()
    missing = sorted(lib - swept - set(kc.EXEMPT))
    assert not missing, "kernel instantiations no sweep case launches (add a case to tests/kernel_cases.py): %s" % missing


def test_the_case_table_names_only_real_kernels(pkg):
    """The table's dispatch model must not drift into naming kernels that do not exist (a typo would cover nothing)."""
    lib = library_kernels(_nm(pkg))
    ghosts = sorted(kc.launched() - lib)
    assert not ghosts, "the case table launches kernels libaesw.so does not have: %s" % ghosts
    assert set(kc.EXEMPT) <= lib
    assert set(kc.EXEMPT) == {"probe_fill_kernel", "probe_fronts_kernel"}


def test_case_table_shape():
    """72 encrypt cases (3 layouts x 2 table paths x 4 key forms x 3 store modes), 18 key_kernel cases, and the counts the
    dispatch model gives per family."""
    assert len(kc.ENCRYPT_CASES) == 72 and len(set(kc.ENCRYPT_CASES)) == 72
    assert len(kc.KEY_CASES) == 18
    fam = {}
    for name in kc.launched():
        f = name.split("<")[0]
        fam[f] = fam.get(f, 0) + 1
    assert fam == {"encrypt_kernel": 72, "key_kernel": 12, "check_kernel": 4, "assemble_kernel": 4,
                   "assemble_fr_oneshot_kernel": 3, "assemble_fr_aligned_kernel": 9, "expand_fr_kernel": 3,
                   "expand_fr_oneshot_kernel": 6, "table_kernel": 1}, fam


def test_dispatch_model_edges():
    assert [kc.auto_waves(l, False) for l in kc.LAYOUTS] == [2, 3, 3]
    assert [kc.auto_waves(l, True) for l in kc.LAYOUTS] == [1, 1, 1]
    assert [kc.auto_waves(l, True, waves_pbk=4) for l in kc.LAYOUTS] == [2, 3, 4]
    assert kc.auto_waves_key(kc.DENSE, True, waves_pbk=4) == 4
    assert kc.effective_remap(3, 7) == 0 and kc.effective_remap(24, 7) == 7 and kc.effective_remap(0, 2) == 2
    assert kc.assemble_kernel_choice(True, 4, 7, 7) == 0 and kc.assemble_kernel_choice(True, 4, 8, 7) == 2
    assert kc.assemble_kernel_choice(False, 1, 16, 10) == 0 and kc.assemble_kernel_choice(True, 1, 7, 7) == 1
