"""CPU: the C ABI of the transform over group elements (include/snarkv_g1_ntt.h): the header is strict C99, both device
libraries export every declared name and only their own, the ctypes table of snark_verifier_amd.g1_ntt lists exactly those names
and shares none with the other tables, and every refusal of the header comes back with its code without a device (the argument
checks come before any HIP call; the context and the key are fake structs)."""
import ctypes
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "snarkv_g1_ntt.h")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402

NAMES = ["g1_ntt_dev", "g1_ntt_max_k", "ipa_dk_lagrange_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import g1_ntt
    from snark_verifier_amd import pallas as PL

    want = sorted(p + n for p in ("snarkv_", "snarkv_pallas_") for n in NAMES)
    assert AU.declared(HDR) == want == sorted(g1_ntt.SIGNATURES)
    others = set()
    for mod, attr in AU.TABLES.items():
        others |= set(getattr(importlib.import_module("snark_verifier_amd." + mod), attr))
    assert not set(want) & others
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("ntt_dev", "intt_dev", "dk_lagrange_dev", "max_k"):
        assert callable(getattr(sv.g1_ntt, fn))
    assert (sv.g1_ntt.FORWARD, sv.g1_ntt.INVERSE) == (sv.ntt.FORWARD, sv.ntt.INVERSE) == (0, 1)


def test_the_cap_is_at_least_20_and_the_one_the_header_states():
    from snark_verifier_amd import g1_ntt

    for pallas in (False, True):
        assert g1_ntt.api(pallas).g1_ntt_max_k() == 22 >= 20
    assert "g1_ntt_max_k(): 22" in open(HDR).read()


def test_every_refusal_comes_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import g1_ntt

    for pallas in (False, True):
        a = g1_ntt.api(pallas)
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        base = 0x100000  # device addresses are only compared here, never followed
        k = 4
        size = 64 << k
        out = base + size

        def call(c=pc, i=base, o=out, kk=k, d=0):
            return a.g1_ntt_dev(c, i, o, kk, d)

        assert call(c=None) == sv.SNARKV_ERR_ARG
        assert call(i=None) == sv.SNARKV_ERR_ARG and call(o=None) == sv.SNARKV_ERR_ARG
        assert call(i=base + 8) == sv.SNARKV_ERR_ARG and call(o=out + 4) == sv.SNARKV_ERR_ARG  # 16-byte alignment
        assert call(d=2) == sv.SNARKV_ERR_ARG and call(d=0xFFFFFFFF) == sv.SNARKV_ERR_ARG
        top = int(a.g1_ntt_max_k())
        assert call(kk=top + 1) == sv.SNARKV_ERR_LENGTH and call(kk=0xFFFFFFFF) == sv.SNARKV_ERR_LENGTH
        # in and out: the same buffer or disjoint; anything between is refused, at either end, whatever the direction
        for d in (0, 1):
            for o in (base + 64, base + size - 64, base - 64, base - size + 64, base + size // 2):
                assert call(o=o, d=d) == sv.SNARKV_ERR_ARG and "overlap" in a.last_error(), o - base
        assert call(i=None, kk=top + 1) == sv.SNARKV_ERR_ARG and call(d=2, kk=top + 1) == sv.SNARKV_ERR_ARG  # arguments before lengths

        # the key: null, another device, a shard (at either end), over the cap, an output inside the key's points
        def lagrange(c=pc, key=None, o=out, **fields):
            f = dict(device=0, k=k, d_points=base, first=0, count=1 << k)
            f.update(fields)
            fk = AU.FakeKey(**f)
            return a.ipa_dk_lagrange_dev(c, ctypes.addressof(fk) if key is None else key, o)

        assert lagrange(c=None) == sv.SNARKV_ERR_ARG and a.ipa_dk_lagrange_dev(pc, None, out) == sv.SNARKV_ERR_ARG
        assert lagrange(o=None) == sv.SNARKV_ERR_ARG and lagrange(o=out + 8) == sv.SNARKV_ERR_ARG
        assert lagrange(device=1) == sv.SNARKV_ERR_ARG and "device" in a.last_error()
        assert lagrange(first=0, count=(1 << k) // 2) == sv.SNARKV_ERR_LENGTH and "shard" in a.last_error()
        assert lagrange(first=(1 << k) // 2, count=(1 << k) // 2) == sv.SNARKV_ERR_LENGTH and "shard" in a.last_error()
        assert lagrange(k=top + 1, count=1 << (top + 1)) == sv.SNARKV_ERR_LENGTH
        assert lagrange(o=base) == sv.SNARKV_ERR_ARG and "overlap" in a.last_error()  # the key is only read
        assert lagrange(o=base + size - 64) == sv.SNARKV_ERR_ARG and "overlap" in a.last_error()
        # (a correct call is not made here: a fake context must never reach the runtime)
