"""CPU: the C ABI of the batched IPA calls (include/snarkv_ipa_batch.h): the header is strict C99 next to the other
product headers, both device libraries export every name it declares, the ctypes table of
snark_verifier_amd.ipa_batch lists exactly those names, the Python wrappers exist, and bad arguments are refused with
the documented codes before any device work."""
import ctypes
import os

import abi_util as AU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_ipa_batch.h")


def test_headers_are_strict_c99():
    for h in ("snarkv_ipa_batch.h", "snarkv_ipa_prover.h", "snarkv_amd.h", "snarkv_pallas.h"):
        AU.assert_strict_c99(h)


def test_both_libraries_export_every_declared_name():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_batch
    from snark_verifier_amd import pallas as PL

    declared = AU.declared(HDR)
    assert len(declared) == 10
    assert sorted(ipa_batch.SIGNATURES) == declared
    assert not set(declared) & AU.other_tables(ipa_batch)  # the other tables stay as they are
    bn, pa = sv.load_library(), PL.load_library()
    for name in declared:
        assert hasattr(pa if "pallas" in name else bn, name), name


def test_python_wrappers_exist():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_batch
    from snark_verifier_amd import pallas as PL

    for cls in (sv.Context, PL.PallasContext):
        assert callable(cls.ipa_commit_batch) and callable(cls.ipa_commit_batch_dev)
    for cls in (sv.IpaDecidingKey, PL.PallasIpaDecidingKey):
        assert callable(cls.prepare) and isinstance(cls.table_bytes, property)
    assert ipa_batch.SHARED_WINDOWS == 32


def test_bad_arguments_are_refused_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_batch

    for pallas in (False, True):
        a = ipa_batch.api(pallas)
        out, b32 = ctypes.create_string_buffer(64), b"\x00" * 32
        assert a.ipa_commit_batch(None, None, b32, 1, 1, out) == sv.SNARKV_ERR_ARG
        assert a.ipa_commit_batch_dev(None, None, None, 1, 1, 0, None) == sv.SNARKV_ERR_ARG
        assert a.ipa_dk_prepare(None, None) == sv.SNARKV_ERR_ARG
        assert a.ipa_dk_table_bytes(None) == 0
        ctx = AU.FakeCtx(device=0)
        whole, shard = AU.FakeKey(device=0, k=3, first=0, count=8), AU.FakeKey(device=0, k=3, first=4, count=4)
        pc, pw, ps = ctypes.addressof(ctx), ctypes.addressof(whole), ctypes.addressof(shard)
        assert a.ipa_commit_batch(pc, pw, b32, 0, 1, out) == sv.SNARKV_ERR_EMPTY    # n = 0
        assert a.ipa_commit_batch(pc, pw, b32, 1, 0, out) == sv.SNARKV_ERR_EMPTY    # m = 0
        assert a.ipa_commit_batch(pc, pw, b32, 9, 1, out) == sv.SNARKV_ERR_LENGTH   # n > count
        assert a.ipa_commit_batch(pc, ps, b32, 1, 1, out) == sv.SNARKV_ERR_LENGTH   # a shard
        assert a.ipa_commit_batch_dev(pc, ps, pc, 1, 1, 0, pc) == sv.SNARKV_ERR_LENGTH
        other = AU.FakeCtx(device=1)
        assert a.ipa_commit_batch(ctypes.addressof(other), pw, b32, 1, 1, out) == sv.SNARKV_ERR_ARG  # key of another device
