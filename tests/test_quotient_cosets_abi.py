"""CPU: the C ABI of the coset-at-a-time quotient (include/snarkv_quotient_cosets.h): the header is strict C99, both device
libraries export every declared name and only their own, the second ctypes table of snark_verifier_amd.quotient lists exactly
those names and shares none with any other table, and every refusal comes back with quotient_dev's code in quotient_dev's
order, without a device (the argument checks come before any HIP call; the context is a fake struct): each refusal is asked
of both calls side by side.  The work buffer is n_cols * n elements: what touches it is "overlap", what only an extended work
buffer would touch is not."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_quotient_cosets.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402
import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
CALLS = ["quotient_cosets_dev", "poly_cosets_join_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import quotient
    from snark_verifier_amd import pallas as PL

    want = sorted(p + c for p in ("snarkv_", "snarkv_pallas_") for c in CALLS)
    declared = [n for n in AU.declared(HDR)]
    assert declared == want == sorted(quotient.COSETS_SIGNATURES)
    assert not set(want) & (AU.other_tables(quotient) | set(quotient.SIGNATURES))
    for hdr in os.listdir(INC):  # no other header declares them
        if hdr.endswith(".h") and hdr != os.path.basename(HDR):
            assert not set(want) & set(AU.declared(os.path.join(INC, hdr))), hdr
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("cosets_dev", "cosets_join_dev"):
        assert callable(getattr(sv.quotient, fn))


def test_every_refusal_is_quotient_devs_and_comes_without_a_device():
    """(a correct call is never made here: a fake context must not reach the runtime)"""
    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt
    from snark_verifier_amd import quotient as Q

    ARG, ENC, EMPTY, LENGTH = sv.SNARKV_ERR_ARG, sv.SNARKV_ERR_ENCODING, sv.SNARKV_ERR_EMPTY, sv.SNARKV_ERR_LENGTH
    for pallas, curve in ((False, "bn254"), (True, "pallas")):
        a, ca = Q.api(pallas), Q.cosets_api(pallas)
        r = FIELD[curve]
        max_k = int(ntt.api(pallas).ntt_max_k())
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
        k, e, n_cols = 4, 2, 3
        col, ext = 32 << k, 32 << (k + e)
        COEFFS, VALS, OUT, WORK, H = ((1 << 44) * i for i in (1, 2, 3, 4, 5))  # only compared, never followed

        def code(instrs):
            return b"".join(Q.pack_instr(*i) for i in instrs)

        good = [(Q.MUL, 0, Q.COL(0), Q.COL(2, -1)), (Q.FMA, 1, Q.REG(0), Q.CONST(1), Q.COL(1, 511)), (Q.SUB, 1, Q.REG(1), Q.REG(0))]
        many = [(Q.ADD, 0, Q.COL(0), Q.COL(1))] * 4097
        ok_c = fe(1) + fe(r - 1)
        faults = {
            "read before write": [(Q.ADD, 0, Q.COL(0), Q.REG(2))],
            "dst 16": [(Q.ADD, 16, Q.COL(0), Q.COL(1))],
            "register 16": [(Q.ADD, 1, Q.REG(16), Q.COL(1))],
            "kind 3": [(Q.ADD, 0, Q.COL(0), 3 << 30)],
            "c on MUL": [(Q.MUL, 0, Q.COL(0), Q.COL(1), Q.CONST(0))],
            "unknown op": [(4, 0, Q.COL(0), Q.COL(1))],
            "zero field": [(Q.ADD, 0, Q.COL(0), Q.COL(1), 0, 1)],
            "column = n_cols": [(Q.ADD, 0, Q.COL(0), Q.COL(n_cols))],
            "constant = n_consts": [(Q.ADD, 0, Q.CONST(2), Q.COL(1))],
        }

        def both(c=pc, i=COEFFS, kk=k, ee=e, nc=n_cols, prog=good, ni=None, cs=ok_c, ncs=2, s=fe(5), si=fe(7), w=WORK, h=H):
            """the same arguments to quotient_dev and to quotient_cosets_dev -> the code both gave, and whether both said
            "overlap" """
            packed = None if prog is None else code(prog)
            args = (c, i, kk, ee, nc, packed, len(prog) if ni is None else ni, cs, ncs, s, si, w, h)
            rc_q = a.quotient_dev(*args)
            msg_q = a.last_error()
            rc_c = ca.quotient_cosets_dev(*args)
            msg_c = ca.last_error()
            assert rc_q == rc_c < 0, (rc_q, rc_c)
            assert ("overlap" in msg_q) == ("overlap" in msg_c) or rc_c != ARG
            return rc_c, rc_c == ARG and "overlap" in msg_c

        def qc(**kw):
            return both(**kw)[0]

        def overlap(**kw):
            return both(**kw)[1]

        assert qc(c=None) == ARG and qc(i=None) == ARG and qc(w=None) == ARG and qc(h=None) == ARG and qc(prog=None, ni=1) == ARG
        assert qc(cs=None) == ARG and qc(s=None) == ARG and qc(si=None) == ARG and qc(s=fe(0)) == ARG and qc(si=fe(0)) == ARG
        assert "shift" in ca.last_error()
        assert qc(i=COEFFS + 8) == ARG and qc(w=WORK + 8) == ARG and qc(h=H + 4) == ARG
        for name, bad in faults.items():
            assert qc(prog=good + bad) == ARG, name
            assert "instruction %d" % len(good) in ca.last_error(), (name, ca.last_error())
        # work (n_cols columns of n), h (N) and the coefficients: pairwise disjoint -- these overlap on both routes
        assert overlap(h=WORK) and overlap(h=WORK + n_cols * col - 32) and overlap(h=WORK - ext + 32)
        assert overlap(w=COEFFS + n_cols * col - 32) and overlap(w=COEFFS - n_cols * col + 32)
        assert overlap(h=COEFFS + 32) and overlap(h=COEFFS - ext + 32) and overlap(w=COEFFS) and overlap(w=H + ext - 32)
        assert qc(cs=fe(r) * 2) == ENC and qc(s=fe(r)) == ENC and qc(si=fe(r + 1)) == ENC
        assert qc(nc=0) == EMPTY and qc(ni=0) == EMPTY
        assert qc(prog=many) == LENGTH and qc(ee=9) == LENGTH and qc(kk=max_k - 1) == LENGTH
        assert qc(cs=fe(1) * 1025, ncs=1025) == LENGTH and qc(nc=(1 << 20) + 1, w=(1 << 61), h=(1 << 58)) == LENGTH
        # the order: arguments, the program, the overlap, the encoding, empty, the lengths
        assert qc(prog=good + faults["kind 3"], s=fe(r)) == ARG and overlap(h=WORK, si=fe(r))
        assert qc(si=fe(r), nc=0) == ENC and qc(si=fe(r), ee=9) == ENC and qc(nc=0, ee=9) == EMPTY
        assert qc(i=None, prog=good + faults["dst 16"]) == ARG and "instruction" not in ca.last_error()
        assert overlap(prog=many, h=WORK) and qc(prog=many + faults["dst 16"], h=WORK) == ARG and "instruction" in ca.last_error()

        # the work buffer is n_cols * n elements, no more: h (or the coefficients) right behind it is no overlap for the coset
        # route -- the next refusal in the order shows that the check was passed -- and is one for quotient_dev
        def cosets(**kw):
            d = dict(c=pc, i=COEFFS, kk=k, ee=e, nc=n_cols, prog=good, cs=ok_c, ncs=2, s=fe(5), si=fe(r), w=WORK, h=H)
            d.update(kw)
            args = (d["c"], d["i"], d["kk"], d["ee"], d["nc"], code(d["prog"]), len(d["prog"]), d["cs"], d["ncs"], d["s"], d["si"],
                    d["w"], d["h"])
            return ca.quotient_cosets_dev(*args), a.quotient_dev(*args), a.last_error()

        for kw in (dict(h=WORK + n_cols * col), dict(i=WORK + n_cols * col), dict(h=WORK + n_cols * ext - 32)):
            rc_c, rc_q, msg_q = cosets(**kw)
            assert rc_c == ENC and rc_q == ARG and "overlap" in msg_q, kw
        rc_c, _, _ = cosets(h=WORK + n_cols * col - 32)  # the last element of work
        assert rc_c == ARG and "overlap" in ca.last_error()
        rc_c, _, _ = cosets(w=H - n_cols * col + 32)  # ... on the first of h
        assert rc_c == ARG and "overlap" in ca.last_error()

        # ---- the join
        def jn(c=pc, i=VALS, kk=k, ee=e, si=fe(7), o=OUT):
            return ca.poly_cosets_join_dev(c, i, kk, ee, si, o)

        assert jn(c=None) == ARG and jn(i=None) == ARG and jn(o=None) == ARG and jn(si=None) == ARG and jn(i=VALS + 8) == ARG
        assert jn(o=OUT + 8) == ARG and jn(si=fe(0)) == ARG and "shift" in ca.last_error()
        for o in (VALS + 32, VALS - 32, VALS + ext - 32, VALS - ext + 32):
            assert jn(o=o) == ARG and "overlap" in ca.last_error(), o - VALS
        assert jn(si=fe(r)) == ENC and jn(ee=9) == LENGTH and jn(kk=max_k, ee=1) == LENGTH and jn(kk=max_k + 1, ee=0) == LENGTH
        assert jn(o=VALS, ee=9) == LENGTH  # in place is allowed, so it reaches the length check
        assert jn(o=VALS + 32, si=fe(r)) == ARG and "overlap" in ca.last_error() and jn(si=fe(r), ee=9) == ENC
