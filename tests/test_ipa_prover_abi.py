"""CPU: the C ABI of the IPA prover (include/snarkv_ipa_prover.h): the header is strict C99, both
libraries export every name it declares, the ctypes table of snark_verifier_amd.ipa_prover lists
exactly those names (and none of snarkv_amd.h's), and null arguments are refused before any device
work."""
import ctypes
import os

import abi_util as AU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "snarkv_ipa_prover.h")


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_every_declared_name():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_prover
    from snark_verifier_amd import pallas as PL

    declared = AU.declared(HDR, r"\b(snarkv_[a-z0-9_]+)\s*\(")
    assert len(declared) == 16
    assert sorted(ipa_prover.SIGNATURES) == declared
    assert not set(declared) & AU.other_tables(ipa_prover)  # the other tables stay as they are
    bn, pa = sv.load_library(), PL.load_library()
    for name in declared:
        assert hasattr(bn if not name.startswith("snarkv_pallas_") else pa, name), name


def test_null_arguments_are_refused_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import _bind, ipa_prover
    from snark_verifier_amd import pallas as PL

    for lib, prefix in ((sv.load_library(), "snarkv_"), (PL.load_library(), "snarkv_pallas_")):
        api = _bind.Api(lib, prefix, ipa_prover._SHAPES)
        b32, b64 = b"\x00" * 32, b"\x00" * 64
        out = ctypes.create_string_buffer(64)
        h = ctypes.c_void_p()
        assert api.ipa_prover_round(None, out, out) == sv.SNARKV_ERR_ARG
        assert api.ipa_prover_fold(None, b32) == sv.SNARKV_ERR_ARG
        assert api.ipa_prover_finish(None, out, out) == sv.SNARKV_ERR_ARG
        api.ipa_prover_destroy(None)
        assert api.ipa_prover_begin(None, None, b32, 1, b32, b64, b32, ctypes.byref(h)) == sv.SNARKV_ERR_ARG
        assert api.ipa_prover_begin_dev(None, None, None, 1, b32, b64, b32, ctypes.byref(h)) == sv.SNARKV_ERR_ARG
        assert api.ipa_commit(None, None, b32, 1, None, None, out) == sv.SNARKV_ERR_ARG
        assert api.ipa_as_combine_dev(None, b32, 1, 1, b32, None, None) == sv.SNARKV_ERR_ARG
