"""CPU: the C ABI of the column products (include/snarkv_poly_prod.h): the header is strict C99, both device libraries export
every declared name and only their own, the ctypes table of snark_verifier_amd.poly_prod lists exactly those names and shares
none with the other tables, and every refusal of the header comes back with its code, in the header's order, without a device
(the argument checks come before any HIP call; the context is a fake struct)."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_poly_prod.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import abi_util as AU  # noqa: E402
import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
CALLS = ["poly_mul_dev", "poly_prod_affine_dev", "poly_batch_invert_dev", "poly_grand_product_dev", "poly_perm_product_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import poly_prod
    from snark_verifier_amd import pallas as PL

    want = sorted(p + c for p in ("snarkv_", "snarkv_pallas_") for c in CALLS)
    assert AU.declared(HDR) == want == sorted(poly_prod.SIGNATURES)
    assert not set(want) & AU.other_tables(poly_prod)
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("mul_dev", "prod_affine_dev", "batch_invert_dev", "grand_product_dev", "perm_product_dev"):
        assert callable(getattr(sv.poly_prod, fn))
    assert sv.poly_prod.NONE == 0xFFFFFFFF
    assert re.search(r"#define SNARKV_POLY_NONE 0xFFFFFFFFu", open(HDR).read())
    assert 2 <= sv.poly_prod.BLOCK <= 1024 and sv.poly_prod.LEVEL_BLOCK >= 2 and sv.poly_prod.AFFINE_TERMS >= 1


def test_the_module_constants_are_the_kernels():
    from snark_verifier_amd import poly_prod

    txt = open(os.path.join(ROOT, "snark-verifier_amd", "csrc", "poly_prod.hip")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, txt).group(1))

    assert poly_prod.BLOCK == const("kProdThreads") * const("kProdLane")
    assert poly_prod.LEVEL_BLOCK == const("kProdThreads")
    assert poly_prod.AFFINE_TERMS == const("kProdAffineTerms")


def _u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def test_every_refusal_comes_without_a_device():
    """(a correct call is never made here: a fake context must not reach the runtime)"""
    import snark_verifier_amd as sv
    from snark_verifier_amd import poly_prod

    ARG, ENC, EMPTY, LENGTH = sv.SNARKV_ERR_ARG, sv.SNARKV_ERR_ENCODING, sv.SNARKV_ERR_EMPTY, sv.SNARKV_ERR_LENGTH
    for pallas, curve in ((False, "bn254"), (True, "pallas")):
        a = poly_prod.api(pallas)
        r = FIELD[curve]
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
        n, n_polys = 48, 4
        size = 32 * n
        # device addresses are only compared here, never followed; 2^40 apart, so that buffers of the refused length
        # 2^30 + 1 (32 GiB and a bit, work twice that, four columns four times) still do not meet
        polys = 1 << 40
        A, B, OUT, WORK, Z, START, EARLIER = (polys * i for i in (1, 2, 3, 4, 6, 7, 8))
        TOTAL = START + 32
        big = (1 << 30) + 1

        def overlap(rc):
            return rc == ARG and "overlap" in a.last_error()

        # ---- mul
        def mul(c=pc, x=A, y=B, nn=n, o=OUT):
            return a.poly_mul_dev(c, x, y, nn, o)

        assert mul(c=None) == ARG and mul(x=None) == ARG and mul(y=None) == ARG and mul(o=None) == ARG
        assert mul(x=A + 8) == ARG and mul(y=B + 4) == ARG and mul(o=OUT + 8) == ARG  # 16-byte alignment
        for o in (A + 32, A - 32, A + size - 32, B + 32, B - size + 32):
            assert overlap(mul(o=o)), o - A
        assert mul(nn=0) == EMPTY and mul(nn=big) == LENGTH
        assert mul(x=None, nn=0) == ARG and overlap(mul(o=A + 32, nn=big))  # the order: arguments before the lengths

        # ---- batch_invert
        def inv(c=pc, i=A, nn=n, o=OUT):
            return a.poly_batch_invert_dev(c, i, nn, o)

        assert inv(c=None) == ARG and inv(i=None) == ARG and inv(o=None) == ARG and inv(i=A + 8) == ARG and inv(o=OUT + 4) == ARG
        for o in (A + 32, A - 32, A + size - 32, A - size + 32):
            assert overlap(inv(o=o)), o - A
        assert inv(nn=0) == EMPTY and inv(nn=big) == LENGTH and inv(i=None, nn=0) == ARG and overlap(inv(o=A + 32, nn=big))

        # ---- grand_product
        def gp(c=pc, f=A, nn=n, s=START, o=OUT, t=TOTAL):
            return a.poly_grand_product_dev(c, f, nn, s, o, t)

        assert gp(c=None) == ARG and gp(f=None) == ARG and gp(o=None) == ARG
        assert gp(f=A + 8) == ARG and gp(o=OUT + 8) == ARG and gp(s=START + 8) == ARG and gp(t=TOTAL + 8) == ARG
        for o in (A + 32, A - 32, A + size - 32, A - size + 32):
            assert overlap(gp(o=o)), o - A
        assert overlap(gp(t=OUT)) and overlap(gp(t=OUT + size - 32)) and overlap(gp(t=A + 32))  # the total in out or in f
        assert overlap(gp(t=A, o=A))
        assert overlap(gp(s=OUT)) and overlap(gp(s=OUT + size - 32)) and overlap(gp(s=TOTAL))  # the start in what is written
        assert overlap(gp(s=A + 32, o=A))
        assert gp(nn=0) == EMPTY and gp(nn=big) == LENGTH and gp(nn=0, s=None, t=None) == EMPTY
        assert gp(f=None, nn=0) == ARG and overlap(gp(o=A + 32, nn=big))
        # allowed, so they reach the length check: out = f, and a start in f when out is elsewhere
        assert gp(o=A, nn=big) == LENGTH and gp(s=A + 32, nn=big) == LENGTH

        # ---- prod_affine
        ia, ib = [0, 1, 1], [2, poly_prod.NONE, 3]
        ok_s = fe(1) + fe(r - 1) + fe(0)

        def pa(c=pc, p=polys, nn=n, np_=n_polys, xa=ia, xb=ib, be=ok_s, ga=ok_s, cnt=3, o=OUT):
            return a.poly_prod_affine_dev(c, p, nn, np_, None if xa is None else _u32(xa), None if xb is None else _u32(xb),
                                          be, ga, cnt, o)

        assert pa(c=None) == ARG and pa(p=None) == ARG and pa(o=None) == ARG and pa(p=polys + 8) == ARG and pa(o=OUT + 8) == ARG
        assert pa(xa=None) == ARG and pa(xb=None) == ARG and pa(be=None) == ARG and pa(ga=None) == ARG
        assert pa(xa=[0, 4, 1]) == ARG and "index" in a.last_error()
        assert pa(xb=[2, 4, 3]) == ARG and pa(xa=[0, poly_prod.NONE, 1]) == ARG  # only idx_b may be NONE
        for o in (polys, polys + 32, polys + size - 32, polys + size, polys + 3 * size + size - 32, polys - size + 32):
            assert overlap(pa(o=o)), o - polys
        assert overlap(pa(xa=[0, 0, 0], xb=[poly_prod.NONE] * 3, o=polys + size - 32))  # column 0's last element
        assert pa(xa=[1, 1, 1], xb=[poly_prod.NONE] * 3, o=polys, nn=big) == LENGTH  # column 0 is not named: no overlap
        assert pa(be=fe(1) + fe(r) + fe(0)) == ENC and pa(ga=fe(1) + fe(2) + b"\xff" * 32) == ENC
        assert pa(cnt=0) == EMPTY and pa(nn=0) == EMPTY and pa(np_=0) == EMPTY and pa(nn=big) == LENGTH
        # the order: an argument error, then the encoding, then empty, then the length
        assert pa(xa=[0, 4, 1], be=fe(r) * 3) == ARG and overlap(pa(o=polys, ga=fe(r) * 3))
        assert pa(be=fe(r) * 3, nn=0) == ENC and pa(be=fe(r) * 3, nn=big) == ENC and pa(be=fe(r) * 3, np_=0) == ENC
        assert pa(nn=0, o=None) == ARG

        # ---- perm_product
        iv, iid, isg = [0, 1], [2, 2], [3, 1]

        def pp(c=pc, p=polys, nn=n, np_=n_polys, v=iv, i=iid, sg=isg, cnt=2, be=fe(5), ga=fe(r - 1), s=START, w=WORK, z=Z,
               t=TOTAL):
            return a.poly_perm_product_dev(c, p, nn, np_, None if v is None else _u32(v), None if i is None else _u32(i),
                                           None if sg is None else _u32(sg), cnt, be, ga, s, w, z, t)

        assert pp(c=None) == ARG and pp(p=None) == ARG and pp(w=None) == ARG and pp(z=None) == ARG
        assert pp(p=polys + 8) == ARG and pp(w=WORK + 8) == ARG and pp(z=Z + 4) == ARG and pp(s=START + 8) == ARG
        assert pp(t=TOTAL + 8) == ARG
        assert pp(v=None) == ARG and pp(i=None) == ARG and pp(sg=None) == ARG and pp(be=None) == ARG and pp(ga=None) == ARG
        assert pp(v=[0, 4]) == ARG and pp(i=[4, 2]) == ARG and pp(sg=[3, poly_prod.NONE]) == ARG
        # work (2n elements), z and the total: disjoint from each other and from every column named
        assert overlap(pp(w=polys + 32)) and overlap(pp(z=polys + 3 * size)) and overlap(pp(t=polys + size))
        assert overlap(pp(w=polys - 2 * size + 32)) and overlap(pp(w=polys - size))  # the second half of work on column 0
        assert overlap(pp(z=WORK)) and overlap(pp(z=WORK + size)) and overlap(pp(z=WORK + 2 * size - 32))
        assert overlap(pp(t=WORK + size)) and overlap(pp(t=Z + size - 32))
        assert overlap(pp(s=Z)) and overlap(pp(s=WORK + 2 * size - 32)) and overlap(pp(s=TOTAL))
        assert pp(be=fe(r)) == ENC and pp(ga=fe(r + 1)) == ENC and pp(ga=b"\xff" * 32) == ENC
        assert pp(cnt=0) == EMPTY and pp(nn=0) == EMPTY and pp(np_=0) == EMPTY and pp(nn=big) == LENGTH
        assert pp(v=[0, 4], be=fe(r)) == ARG and overlap(pp(z=WORK, be=fe(r)))
        assert pp(be=fe(r), cnt=0) == ENC and pp(be=fe(r), nn=big) == ENC and pp(cnt=0, nn=big) == EMPTY
        # a start in an earlier z (memory this call does not write), no total: allowed, so it reaches the length check
        assert pp(s=EARLIER, t=None, nn=big) == LENGTH and pp(s=None, nn=big) == LENGTH
