"""Every kernel instantiation in libaesw.so, in any namespace, is launched by a GPU sweep (CPU: reads `nm -C` only).

tests/test_instantiation_coverage.py covers the aesw:: kernels through tests/kernel_cases.py; the many-circuit kernels of
namespace aesw_circ are launched by tests/test_gpu_circuits.py, whose case list is tests/circuit_cases.py."""
import circuit_cases as cc
import kernel_cases as kc
from check_library import all_kernels, nm


def _nm(pkg):
    return nm(pkg.api.LIB_PATH, "-C")


def test_all_kernels_parse():
    text = ("000000000024d470 W void aesw::__device_stub__key_kernel<0, false, 0>(aesw::KeyParams)\n"
            "000000000024d480 W void aesw_circ::__device_stub__circuit_assemble_kernel<true>(aesw_circ::CircAsmParams)\n"
            "0000000000236960 T __device_stub__free_kernel(unsigned char*)\n"
            "000000000026f8e8 V void aesw::key_kernel<0, false, 0>(aesw::KeyParams)\n")
    assert all_kernels(text) == {("aesw", "key_kernel<0,false,0>"), ("aesw_circ", "circuit_assemble_kernel<true>"), ("", "free_kernel")}


def test_every_kernel_in_every_namespace_is_swept(pkg):
    lib = all_kernels(_nm(pkg))
    assert len(lib) >= 100, sorted(lib)[:5]
    old = kc.launched() | set(kc.EXEMPT)
    missing = sorted("%s::%s" % (ns, name) if ns else name for ns, name in lib
                     if not (ns == "aesw" and name in old) and ("%s::%s" % (ns, name)) not in cc.launched())
    assert not missing, "kernel instantiations no sweep launches: %s" % missing


def test_the_circuit_case_list_names_exactly_the_aesw_circ_kernels(pkg):
    lib = {"%s::%s" % (ns, name) for ns, name in all_kernels(_nm(pkg)) if ns == "aesw_circ"}
    assert cc.launched() == lib
    assert cc.launched() == {"aesw_circ::circuit_assemble_kernel<true>", "aesw_circ::circuit_assemble_kernel<false>"}


def test_case_list_shape():
    ks = {k for k, _n, _c in cc.SHAPES}
    assert min(ks) == 7 and max(ks) == 16
    assert {n for _k, n, _c in cc.SHAPES} == {1, 3} and {c for _k, _n, c in cc.SHAPES} == {1, 3, 37}
