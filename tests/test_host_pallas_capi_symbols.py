"""CPU: the two headers of the pallas verification path -- include/snarkv_pallas_decompress.h (libsnarkv_pallas.so) and
include/snarkv_host_pallas.h (libsnarkv_host_pallas.so, the product C API of the pasta flavour of the host mirror) --
are strict C99, the libraries export every name they declare, the product library carries no test hook, the ctypes
tables list exactly the declared names, and argument errors come back as codes without a device."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_util as AU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def host_lib():
    """libsnarkv_host_pallas.so, built the way the test-hook library is: through build.py"""
    import importlib.util

    from snark_verifier_amd import host_api_pallas as HP
    from snark_verifier_amd import pallas as PL

    PL.load_library()
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert os.path.basename(b.build_host_api_pallas()) == "libsnarkv_host_pallas.so"
    return HP.load_library()


@pytest.mark.parametrize("header", ["snarkv_pallas_decompress.h", "snarkv_host_pallas.h"])
def test_new_headers_are_strict_c99(header):
    AU.assert_strict_c99(header)


def test_pallas_library_exports_the_decompression_entry_points():
    from snark_verifier_amd import pallas as PL

    declared = AU.declared(os.path.join(INC, "snarkv_pallas_decompress.h"), r"\b((?:snarkv_)?pallas_[a-z0-9_]+)\s*\(")
    assert declared == ["pallas_g1_decompress", "snarkv_pallas_ctx_set_flags", "snarkv_pallas_g1_decompress"]
    lib = PL.load_library()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name  # bound by pallas.py's table
    assert hasattr(PL.PallasContext, "g1_decompress")


def test_host_pallas_library_exports_exactly_the_declared_names(host_lib):
    from snark_verifier_amd import host_api_pallas as HP

    declared = AU.declared(os.path.join(INC, "snarkv_host_pallas.h"), r"\b(snarkv_host_pallas_[a-z0-9_]+)\s*\(")
    assert len(declared) == 11
    for name in declared:
        assert hasattr(host_lib, name), name
    assert sorted(HP._SIGNATURES) == declared
    r = subprocess.run(["nm", "-D", "--defined-only", host_lib._name], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {f[-1] for f in (line.split() for line in r.stdout.splitlines()) if f}
    assert sorted(s for s in exported if s.startswith("snarkv_host")) == declared  # and nothing of the BN254 API
    assert not [s for s in exported if re.match(r"h[pd]_", s)]  # no test hook in the product library
    hooks = ctypes.CDLL(os.path.join(ROOT, "snark-verifier_amd", "libsnarkv_hosttest_pallas.so"))
    assert hasattr(hooks, "hp_plonk_ipa_point_offsets") and not hasattr(hooks, "snarkv_host_pallas_aggregate")
    import snark_verifier_amd as sv

    assert sv.host_api_pallas is HP
    assert HP.DEVICE_MIN == int(re.search(r"#define SNARKV_HOST_PALLAS_DEVICE_MIN (\d+)",
                                          open(os.path.join(INC, "snarkv_host_pallas.h")).read()).group(1))


def test_host_pallas_argument_errors_without_device(host_lib):
    from snark_verifier_amd import host_api_pallas as HP

    L = host_lib
    h = ctypes.c_void_p()
    assert L.snarkv_host_pallas_protocol_parse(None, 0, ctypes.byref(h)) == HP.ERR_ARG
    assert L.snarkv_host_pallas_protocol_parse(b"\x01\x02", 2, None) == HP.ERR_ARG
    assert L.snarkv_host_pallas_protocol_parse(b"\x01\x02", 2, ctypes.byref(h)) == HP.ERR_PANIC and not h.value
    assert b"truncated" in L.snarkv_host_pallas_last_error()
    with pytest.raises(HP.HostError) as e:
        HP.Protocol(b"\x00" * 7)
    assert e.value.code == HP.ERR_PANIC
    assert L.snarkv_host_pallas_ipa_dk_create(4, None, bytes(64), None, ctypes.byref(h)) == HP.ERR_ARG
    assert L.snarkv_host_pallas_ipa_dk_create(0, bytes(64), bytes(64), None, ctypes.byref(h)) == HP.ERR_ARG
    assert L.snarkv_host_pallas_ipa_decide_all(None, None, 0, None) == HP.ERR_ARG
    assert L.snarkv_host_pallas_ipa_as_create_proof(None, None, 0, None, 0, None, 0, None, None) == HP.ERR_ARG
    assert L.snarkv_host_pallas_ipa_as_verify(None, None, 0, None, 0, None) == HP.ERR_ARG
    # an unknown route is reported as such, whatever else is wrong with the call
    for bad in (3, -1, 99):
        assert L.snarkv_host_pallas_plonk_verify(None, None, None, 0, None, 0, 0, 0, bad) == HP.ERR_ARG
        assert b"route" in L.snarkv_host_pallas_last_error()
        assert L.snarkv_host_pallas_plonk_succinct_verify_batch(None, None, None, 0, None, 0, 0, 0, bad, None, 0) == HP.ERR_ARG
        assert b"route" in L.snarkv_host_pallas_last_error()
        assert L.snarkv_host_pallas_aggregate(None, None, None, 0, None, 0, 1, 0, bad, None, 0, None, None, 0, None, None) == HP.ERR_ARG
        assert b"route" in L.snarkv_host_pallas_last_error()
    for good in (HP.DECOMPRESS_HOST, HP.DECOMPRESS_DEVICE, HP.DECOMPRESS_AUTO):
        assert L.snarkv_host_pallas_plonk_verify(None, None, None, 0, None, 0, 0, 0, good) == HP.ERR_ARG
        assert b"null" in L.snarkv_host_pallas_last_error()
    L.snarkv_host_pallas_protocol_free(None)
    L.snarkv_host_pallas_ipa_dk_free(None)
