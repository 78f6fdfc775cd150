"""CPU: the C ABI of the one-call IPA proof (include/snarkv_ipa_create.h, include/snarkv_host_pallas_prove.h): the headers
are strict C99, both device libraries export every declared name, the ctypes table of snark_verifier_amd.ipa_create lists
exactly those names and shares none with the other tables, the Python wrappers exist, bad arguments are refused with the
documented codes before any device work, and the host library exports exactly its declared names."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_ipa_create.h")
HOST_HDR = os.path.join(INC, "snarkv_host_pallas_prove.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import abi_util as AU  # noqa: E402


def test_headers_are_strict_c99():
    for h in (HDR, HOST_HDR):
        AU.assert_strict_c99(h)


def test_both_libraries_export_every_declared_name():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_create
    from snark_verifier_amd import pallas as PL

    declared = AU.declared(HDR)
    assert declared == ["bn254_ipa_create_proof", "pallas_ipa_create_proof", "snarkv_ipa_create_proof",
                        "snarkv_ipa_create_proof_dev", "snarkv_pallas_ipa_create_proof", "snarkv_pallas_ipa_create_proof_dev"]
    assert sorted(ipa_create.SIGNATURES) == declared
    assert not set(declared) & AU.other_tables(ipa_create)
    bn, pa = sv.load_library(), PL.load_library()
    for name in declared:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name


def test_python_wrappers_exist():
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api_pallas as HP
    from snark_verifier_amd import pallas as PL

    for cls in (sv.Context, PL.PallasContext):
        assert callable(cls.ipa_create_proof)
    for fn in ("create_proof", "create_proof_dev", "create_proof_default", "proof_bytes"):
        assert callable(getattr(sv.ipa_create, fn))
    assert sv.ipa_create.proof_bytes(10, False) == 704 and sv.ipa_create.proof_bytes(10, True) == 768
    assert callable(HP.ipa_create_proof) and callable(HP.load_prove_library)


def test_bad_arguments_are_refused_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_create

    for pallas in (False, True):
        a = ipa_create.api(pallas)
        b32, b64, coeffs = b"\x00" * 32, b"\x01" * 64, b"\x00" * (32 * 8)
        proof, xi, u = ctypes.create_string_buffer(b"\xaa" * 512, 512), ctypes.create_string_buffer(96), ctypes.create_string_buffer(64)
        plen = ctypes.c_size_t(7)
        ctx = AU.FakeCtx(device=0)
        whole, shard = AU.FakeKey(device=0, k=3, first=0, count=8), AU.FakeKey(device=0, k=3, first=4, count=4)
        pc, pw, ps = ctypes.addressof(ctx), ctypes.addressof(whole), ctypes.addressof(shard)

        def call(fn=a.ipa_create_proof, c=pc, dk=pw, h=b64, s=None, p=coeffs, n=8, z=b32, om=None, pbar=None, omb=None, ab=None,
                 ablen=0, out=proof, cap=512, ln=ctypes.byref(plen), x=xi, uu=u):
            return fn(c, dk, h, s, p, n, z, om, pbar, omb, ab, ablen, out, cap, ln, x, uu)

        # null arguments
        assert call(c=None) == sv.SNARKV_ERR_ARG and call(dk=None) == sv.SNARKV_ERR_ARG and call(h=None) == sv.SNARKV_ERR_ARG
        assert call(p=None) == sv.SNARKV_ERR_ARG and call(z=None) == sv.SNARKV_ERR_ARG and call(out=None) == sv.SNARKV_ERR_ARG
        assert call(ln=None) == sv.SNARKV_ERR_ARG and call(x=None) == sv.SNARKV_ERR_ARG and call(uu=None) == sv.SNARKV_ERR_ARG
        assert call(ablen=5) == sv.SNARKV_ERR_ARG  # absorbed bytes announced, none given
        assert call(fn=a.ipa_create_proof_dev, p=None) == sv.SNARKV_ERR_ARG
        # a partial zk set, every way round
        full = dict(s=b64, om=b32, pbar=coeffs, omb=b32)
        for drop in full:
            assert call(**{k: v for k, v in full.items() if k != drop}) == sv.SNARKV_ERR_ARG, drop
            assert call(**{drop: full[drop]}) == sv.SNARKV_ERR_ARG, drop
        # proof_cap too small: the needed length comes back, nothing else is written
        assert call(cap=64 * 3 + 63) == sv.SNARKV_ERR_LENGTH and plen.value == 64 * 3 + 64
        assert call(cap=64 * 3 + 127, **full) == sv.SNARKV_ERR_LENGTH and plen.value == 64 * 3 + 128
        assert proof.raw == b"\xaa" * 512
        # the key and n: a shard, n that is not the key's 2^k, a context on another device
        assert call(dk=ps) == sv.SNARKV_ERR_LENGTH and plen.value == 0
        assert call(n=4) == sv.SNARKV_ERR_LENGTH
        other = AU.FakeCtx(device=1)
        assert call(c=ctypes.addressof(other)) == sv.SNARKV_ERR_ARG


def _build():
    import importlib.util

    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_the_host_library_of_the_one_call_proof():
    """libsnarkv_host_pallas_prove.so exports exactly the names its header declares, the ctypes table of host_api_pallas
    lists them apart from the other two tables, and argument errors come back as codes without a device"""
    from snark_verifier_amd import host_api_pallas as HP

    declared = AU.declared(HOST_HDR, r"\b(snarkv_host_pallas_[a-z0-9_]+)\s*\(")
    assert declared == ["snarkv_host_pallas_ipa_create_proof", "snarkv_host_pallas_prove_last_error"]
    assert sorted(HP._PROVE_SIGNATURES) == declared
    assert not set(declared) & (set(HP._SIGNATURES) | set(HP._FOLD_SIGNATURES))
    assert os.path.basename(_build().build_host_api_pallas_prove()) == "libsnarkv_host_pallas_prove.so"
    L = HP.load_prove_library()
    r = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {f[-1] for f in (line.split() for line in r.stdout.splitlines()) if f}
    assert sorted(s for s in exported if s.startswith("snarkv_")) == declared
    ln = ctypes.c_size_t(0)
    assert L.snarkv_host_pallas_ipa_create_proof(None, None, 0, None, None, None, None, None, 0, None, 0, ctypes.byref(ln), None) == HP.ERR_ARG
    assert b"null" in L.snarkv_host_pallas_prove_last_error()
