"""CPU: the C ABI of the blinded batch commitment (include/snarkv_ipa_commit_blinded.h): the header is strict C99, both device
libraries export the names it declares, the ctypes table of snark_verifier_amd.ipa_commit_blinded lists exactly those, no
other table names them, and bad arguments are refused with the documented codes before any device work."""
import ctypes
import os

import abi_util as AU

HDR = os.path.join(AU.INC, "snarkv_ipa_commit_blinded.h")
NAMES = ["snarkv_ipa_commit_blinded_batch_dev", "snarkv_pallas_ipa_commit_blinded_batch_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99("snarkv_ipa_commit_blinded.h")


def test_both_libraries_export_the_declared_names():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_commit_blinded as CB
    from snark_verifier_amd import pallas as PL

    assert AU.declared(HDR) == NAMES == sorted(CB.SIGNATURES)
    others = set()
    for mod, attr in AU.TABLES.items():
        others |= set(getattr(__import__("snark_verifier_amd." + mod, fromlist=[attr]), attr))
    assert not others & set(NAMES)
    assert AU.declared(os.path.join(AU.INC, "snarkv_ipa_batch.h")) == sorted(sv.ipa_batch.SIGNATURES)  # that header is as it was
    bn, pa = sv.load_library(), PL.load_library()
    assert hasattr(bn, NAMES[0]) and not hasattr(bn, NAMES[1])
    assert hasattr(pa, NAMES[1]) and not hasattr(pa, NAMES[0])
    assert callable(sv.ipa_commit_blinded.commit_blinded_batch_dev)
    res, args = CB.SIGNATURES[NAMES[0]]
    assert res is ctypes.c_int and len(args) == 9  # ctx, dk, s64, d_polys32, n, m, blinds32, slices, d_out64s


def test_bad_arguments_are_refused_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_commit_blinded as CB

    for pallas in (False, True):
        a = CB.api(pallas)
        f = a.ipa_commit_blinded_batch_dev
        ctx, other = AU.FakeCtx(device=0), AU.FakeCtx(device=1)
        whole, shard = AU.FakeKey(device=0, k=3, first=0, count=8), AU.FakeKey(device=0, k=3, first=4, count=4)
        pc, po, pw, ps = (ctypes.addressof(x) for x in (ctx, other, whole, shard))
        s64, b32 = b"\x01" + b"\x00" * 63, b"\x00" * 32
        assert f(None, pw, s64, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ARG
        assert f(pc, None, s64, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ARG
        assert f(pc, pw, None, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ARG      # no S
        assert f(pc, pw, s64, None, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ARG
        assert f(pc, pw, s64, pc, 1, 1, None, 0, pc) == sv.SNARKV_ERR_ARG      # no blinds
        assert f(pc, pw, s64, pc, 1, 1, b32, 0, None) == sv.SNARKV_ERR_ARG
        assert f(po, pw, s64, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ARG       # key of another device
        assert f(pc, pw, s64, pc, 0, 1, b32, 0, pc) == sv.SNARKV_ERR_EMPTY     # n = 0
        assert f(pc, pw, s64, pc, 1, 0, b32, 0, pc) == sv.SNARKV_ERR_EMPTY     # m = 0
        assert f(pc, pw, s64, pc, 9, 1, b32, 0, pc) == sv.SNARKV_ERR_LENGTH    # n > 2^k
        assert f(pc, ps, s64, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_LENGTH    # a shard
        assert f(pc, pw, b"\x00" * 64, pc, 1, 1, b32, 0, pc) == sv.SNARKV_ERR_ENCODING  # S at infinity
        assert "infinity" in a.last_error()
