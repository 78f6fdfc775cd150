"""CPU: the C ABI of the transform (include/snarkv_ntt.h): the header is strict C99, both device libraries export every
declared name and only their own, the ctypes table of snark_verifier_amd.ntt lists exactly those names and shares none with the
other tables, every refusal of the header comes back with its code without a device (the argument checks come before any HIP
call; the context is a fake struct), and the generated root of unity is the oracle's."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_ntt.h")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402
import ntt_util as U  # noqa: E402


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt
    from snark_verifier_amd import pallas as PL

    want = sorted(["snarkv_ntt_dev", "snarkv_ntt_max_k", "snarkv_pallas_ntt_dev", "snarkv_pallas_ntt_max_k"])
    assert AU.declared(HDR) == want == sorted(ntt.SIGNATURES)
    assert not set(want) & AU.other_tables(ntt)
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("ntt_dev", "intt_dev", "max_k", "passes"):
        assert callable(getattr(sv.ntt, fn))
    assert sv.ntt.TILE_BITS == 9 and (sv.ntt.FORWARD, sv.ntt.INVERSE) == (0, 1)
    assert [sv.ntt.passes(k) for k in (0, 9, 10, 14, 15, 21, 22, 28, 29, 30)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


def test_max_k_is_the_smaller_of_the_two_adicity_and_30():
    from snark_verifier_amd import ntt

    assert ntt.api(False).ntt_max_k() == 28 == min(U.BN.TWO_ADICITY, 30)
    assert ntt.api(True).ntt_max_k() == 30 == min(U.PA.TWO_ADICITY, 30)


def test_every_refusal_comes_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt

    for pallas, curve in ((False, "bn254"), (True, "pallas")):
        a = ntt.api(pallas)
        r = U.CURVES[curve].R
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        base = 0x100000  # device addresses are only compared here, never followed
        k, count = 4, 3
        size = 32 * count << k
        out = base + size
        fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731

        def call(c=pc, i=base, o=out, kk=k, n=count, d=0, s=None):
            return a.ntt_dev(c, i, o, kk, n, d, s)

        assert call(c=None) == sv.SNARKV_ERR_ARG
        assert call(i=None) == sv.SNARKV_ERR_ARG and call(o=None) == sv.SNARKV_ERR_ARG
        assert call(i=base + 8) == sv.SNARKV_ERR_ARG and call(o=out + 4) == sv.SNARKV_ERR_ARG  # 16-byte alignment
        assert call(d=2) == sv.SNARKV_ERR_ARG and call(d=0xFFFFFFFF) == sv.SNARKV_ERR_ARG
        assert call(s=fe(0)) == sv.SNARKV_ERR_ARG and "zero" in a.last_error()
        assert call(s=fe(r)) == sv.SNARKV_ERR_ENCODING and call(s=fe(r + 1)) == sv.SNARKV_ERR_ENCODING
        assert call(s=b"\xff" * 32) == sv.SNARKV_ERR_ENCODING
        assert call(n=0) == sv.SNARKV_ERR_EMPTY
        top = int(a.ntt_max_k())
        assert call(kk=top + 1) == sv.SNARKV_ERR_LENGTH and call(kk=0xFFFFFFFF) == sv.SNARKV_ERR_LENGTH
        assert call(n=65536) == sv.SNARKV_ERR_LENGTH
        # in and out: the same buffer or disjoint; anything between is refused, at either end, whatever the direction
        for d in (0, 1):
            for o in (base + 32, base + size - 32, base - 32, base - size + 32, base + 32 * (1 << k)):
                assert call(o=o, d=d) == sv.SNARKV_ERR_ARG and "overlap" in a.last_error(), o - base
        # the order of the table: an argument error before the lengths, the shift before the overlap
        assert call(i=None, n=0) == sv.SNARKV_ERR_ARG and call(d=2, kk=top + 1) == sv.SNARKV_ERR_ARG
        # (a correct call is not made here: a fake context must never reach the runtime)


def test_the_generated_root_of_unity_is_the_oracles():
    csrc = os.path.join(ROOT, "snark-verifier_amd", "csrc")
    for curve, hdr in (("bn254", "bn254_consts.h"), ("pallas", "pallas_consts.h")):
        cv = U.CURVES[curve]
        txt = open(os.path.join(csrc, hdr)).read()

        def val(name):
            m = re.search(r"#define %s \{([^}]*)\}" % name, txt)
            return sum(int(x, 16) << (29 * i) for i, x in enumerate(m.group(1).split(",")))

        assert int(re.search(r"#define SNARKV_FR_TWO_ADICITY (\d+)", txt).group(1)) == cv.TWO_ADICITY
        root = U.omega(curve, cv.TWO_ADICITY)
        assert val("SNARKV_FR29_ROOT_OF_UNITY_LIMBS") == root * (1 << 261) % cv.R
        assert val("SNARKV_FR29_ROOT_OF_UNITY_INV_LIMBS") == pow(root, -1, cv.R) * (1 << 261) % cv.R
