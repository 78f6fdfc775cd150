"""CPU: the C ABI of the folded IPA decide (include/snarkv_ipa_fold.h): the header is strict C99, both device libraries
export every name it declares, the ctypes table of snark_verifier_amd.ipa_fold lists exactly those names, the Python
wrappers exist, bad arguments are refused with the documented codes before any device work -- and the host-side derivation
of a challenge (`ipa_fold.fold_challenge`, no device work) against the layout it documents."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_ipa_fold.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import abi_util as AU  # noqa: E402


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_every_declared_name():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_fold
    from snark_verifier_amd import pallas as PL

    declared = AU.declared(HDR)
    assert declared == ["bn254_ipa_decide_folded", "pallas_ipa_decide_folded", "snarkv_ipa_decide_folded",
                        "snarkv_ipa_fold_coeffs_dev", "snarkv_pallas_ipa_decide_folded", "snarkv_pallas_ipa_fold_coeffs_dev"]
    assert sorted(ipa_fold.SIGNATURES) == declared
    assert not set(declared) & AU.other_tables(ipa_fold)
    bn, pa = sv.load_library(), PL.load_library()
    for name in declared:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name


def test_python_wrappers_exist():
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    assert sv.ipa_fold.FOLD_BLOCK_BITS == 3
    for cls in (sv.Context, PL.PallasContext):
        assert callable(cls.ipa_decide_folded) and callable(cls.ipa_fold_coeffs_dev)
    assert callable(sv.ipa_fold.fold_challenge) and callable(sv.ipa_fold.decide_folded_default)


def test_bad_arguments_are_refused_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_fold

    for pallas in (False, True):
        a = ipa_fold.api(pallas)
        ok, b32, b64 = ctypes.c_int(7), b"\x00" * 32, b"\x00" * 64
        assert a.ipa_decide_folded(None, None, b32, b64, 1, b32, ctypes.byref(ok)) == sv.SNARKV_ERR_ARG
        assert a.ipa_fold_coeffs_dev(None, 3, b32, 1, b32, 0, None) == sv.SNARKV_ERR_ARG
        ctx = AU.FakeCtx(device=0)
        whole, shard = AU.FakeKey(device=0, k=3, first=0, count=8), AU.FakeKey(device=0, k=3, first=4, count=4)
        pc, pw, ps = ctypes.addressof(ctx), ctypes.addressof(whole), ctypes.addressof(shard)
        assert a.ipa_decide_folded(pc, pw, b32, b64, 1, b32, None) == sv.SNARKV_ERR_ARG       # nowhere to put the verdict
        assert a.ipa_decide_folded(pc, pw, b32, b64, 0, b32, ctypes.byref(ok)) == sv.SNARKV_ERR_EMPTY   # m = 0
        assert ok.value == 0                                                                   # never left as it was
        assert a.ipa_decide_folded(pc, ps, b32, b64, 1, b32, ctypes.byref(ok)) == sv.SNARKV_ERR_LENGTH  # a shard
        other = AU.FakeCtx(device=1)
        assert a.ipa_decide_folded(ctypes.addressof(other), pw, b32, b64, 1, b32, ctypes.byref(ok)) == sv.SNARKV_ERR_ARG
        assert a.ipa_fold_coeffs_dev(pc, 3, b32, 0, b32, 0, pc) == sv.SNARKV_ERR_EMPTY         # m = 0
        assert a.ipa_fold_coeffs_dev(pc, 0, b32, 1, b32, 0, pc) == sv.SNARKV_ERR_LENGTH        # k = 0
        assert a.ipa_fold_coeffs_dev(pc, 29, b32, 1, b32, 0, pc) == sv.SNARKV_ERR_LENGTH       # k > 28
        assert a.ipa_fold_coeffs_dev(pc, 3, b32, 1, b32, 0, pc + 8) == sv.SNARKV_ERR_ARG       # d_h32 not 16-byte aligned


def _build():
    import importlib.util

    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_the_host_library_of_the_folded_decide():
    """include/snarkv_host_pallas_fold.h is strict C99, libsnarkv_host_pallas_fold.so exports exactly the names it
    declares, the ctypes table of host_api_pallas lists them, and argument errors come back as codes without a device"""
    from snark_verifier_amd import host_api_pallas as HP

    hdr = os.path.join(INC, "snarkv_host_pallas_fold.h")
    AU.assert_strict_c99(hdr)
    declared = AU.declared(hdr, r"\b(snarkv_host_pallas_[a-z0-9_]+)\s*\(")
    assert declared == ["snarkv_host_pallas_fold_last_error", "snarkv_host_pallas_ipa_decide_all_folded",
                        "snarkv_host_pallas_ipa_fold_challenge", "snarkv_host_pallas_plonk_verify_folded"]
    assert sorted(HP._FOLD_SIGNATURES) == declared and not set(declared) & set(HP._SIGNATURES)
    assert os.path.basename(_build().build_host_api_pallas_fold()) == "libsnarkv_host_pallas_fold.so"
    L = HP.load_fold_library()
    r = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {f[-1] for f in (line.split() for line in r.stdout.splitlines()) if f}
    assert sorted(s for s in exported if s.startswith("snarkv_")) == declared
    for fn in ("ipa_fold_challenge", "ipa_decide_all_folded", "plonk_verify_folded"):
        assert callable(getattr(HP, fn))
    rho = ctypes.create_string_buffer(32)
    assert L.snarkv_host_pallas_ipa_fold_challenge(None, b"", 0, None, rho) == HP.ERR_ARG
    assert b"null" in L.snarkv_host_pallas_fold_last_error()
    assert L.snarkv_host_pallas_ipa_decide_all_folded(None, None, 0, None, None) == HP.ERR_ARG
    for bad in (3, -1):
        assert L.snarkv_host_pallas_plonk_verify_folded(None, None, None, 0, None, 0, 0, 0, bad, None) == HP.ERR_ARG
        assert b"route" in L.snarkv_host_pallas_fold_last_error()
    assert L.snarkv_host_pallas_plonk_verify_folded(None, None, None, 0, None, 0, 0, 0, HP.DECOMPRESS_AUTO, None) == HP.ERR_ARG


class _FakeHostKey:
    """what `host_api_pallas.ipa_fold_challenge` reads of a key handle"""

    def __init__(self, handle, k):
        self._h, self.k, self.acc_bytes = handle, k, 32 * k + 64


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("seeded", [False, True])
def test_fold_challenge_of_the_host_library_against_hashlib(m, seeded):
    """the C derivation (host/capi_pallas_fold.cpp: the mirror's own BLAKE2b and the reduction of its Blake2b transcript)
    against hashlib and big-integer reduction.  The host key handle begins with its `IpaDecidingKey`, whose first field is
    svk.k: the challenge reads nothing else of it, so a handle made of that one word stands in for a key (a real one
    uploads its points to a device).  It also equals the Python derivation of `ipa_fold.fold_challenge`."""
    import pallas as PA

    from snark_verifier_amd import host_api_pallas as HP
    from snark_verifier_amd import ipa_fold

    _build().build_host_api_pallas_fold()
    k = 5
    rnd = random.Random("fold-challenge-c-%d-%d" % (m, seeded))
    # digests whose halves reach above r are what the reduction is about: random bytes for u make every digest different
    accs = b"".join(b"".join(rnd.randrange(PA.R).to_bytes(32, "little") for _ in range(k)) + rnd.randbytes(64) for _ in range(m))
    seed = rnd.randbytes(32) if seeded else None
    want = hashlib.blake2b((k).to_bytes(4, "little") + (m).to_bytes(4, "little") + accs + (seed or b""), digest_size=64,
                           person=b"snarkv_ipa_fold1").digest()
    want = (int.from_bytes(want, "little") % PA.R).to_bytes(32, "little")
    fake = (ctypes.c_uint64 * 64)()
    fake[0] = k
    key = _FakeHostKey(ctypes.c_void_p(ctypes.addressof(fake)), k)
    assert HP.ipa_fold_challenge(key, accs, seed) == want
    assert HP.ipa_fold_challenge(key, accs, None if seeded else bytes(32)) != want  # the seed is part of the hash
    stride = 32 * k + 64
    xi = b"".join(accs[a * stride:a * stride + 32 * k] for a in range(m))
    u = b"".join(accs[a * stride + 32 * k:(a + 1) * stride] for a in range(m))
    assert ipa_fold.fold_challenge(k, xi, u, True, seed) == want


@pytest.mark.parametrize("pallas", [False, True])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("seeded", [False, True])
def test_fold_challenge_is_blake2b_over_the_accumulators(pallas, m, seeded):
    """the layout that is hashed, written out a second way: one buffer of `k x xi | u` per accumulator"""
    import bn254 as BN
    import pallas as PA

    from snark_verifier_amd import ipa_fold

    k, r = 5, (PA.R if pallas else BN.R)
    assert r == (ipa_fold.R_PALLAS if pallas else ipa_fold.R_BN254)
    rnd = random.Random("fold-challenge-%d-%d" % (m, seeded))
    xis = [b"".join(rnd.randrange(r).to_bytes(32, "little") for _ in range(k)) for _ in range(m)]
    us = [rnd.randbytes(64) for _ in range(m)]
    seed = rnd.randbytes(32) if seeded else None
    accs = b"".join(x + u for x, u in zip(xis, us))
    want = hashlib.blake2b((k).to_bytes(4, "little") + (m).to_bytes(4, "little") + accs + (seed or b""), digest_size=64,
                           person=b"snarkv_ipa_fold1").digest()
    want = (int.from_bytes(want, "little") % r).to_bytes(32, "little")
    assert ipa_fold.fold_challenge(k, b"".join(xis), b"".join(us), pallas, seed) == want
    assert ipa_fold.fold_challenge(k, b"".join(xis), b"".join(us), pallas, None if seeded else bytes(32)) != want  # the seed counts
    assert ipa_fold.fold_challenge(k, b"".join(xis), b"".join(us), not pallas, seed) != want
