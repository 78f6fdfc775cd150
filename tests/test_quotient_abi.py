"""CPU: the C ABI of the quotient calls (include/snarkv_quotient.h): the header is strict C99, both device libraries export
every declared name and only their own, the ctypes table of snark_verifier_amd.quotient lists exactly those names and shares
none with the other tables, the operand macros of the header and the helpers of the module give the same words (a small C
program prints them), and every refusal of the header comes back with its code, in the header's order, without a device (the
argument checks come before any HIP call; the context is a fake struct)."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_quotient.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import abi_util as AU  # noqa: E402
import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
CALLS = ["poly_extend_dev", "quotient_eval_dev", "poly_div_vanishing_dev", "quotient_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import quotient
    from snark_verifier_amd import pallas as PL

    want = sorted(p + c for p in ("snarkv_", "snarkv_pallas_") for c in CALLS)
    assert AU.declared(HDR) == want == sorted(quotient.SIGNATURES)
    assert not set(want) & AU.other_tables(quotient)
    for hdr in ("snarkv_amd.h", "snarkv_pallas.h"):  # the two pinned headers do not declare them
        assert not set(want) & set(AU.declared(os.path.join(INC, hdr)))
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("extend_dev", "eval_dev", "div_vanishing_dev", "quotient_dev", "REG", "CONST", "COL", "Program"):
        assert callable(getattr(sv.quotient, fn))


def test_the_macros_of_the_header_and_the_helpers_of_the_module_agree(tmp_path):
    from snark_verifier_amd import quotient as Q

    operands = [("SNARKV_QUOT_REG(%d)" % i, Q.REG(i)) for i in (0, 7, 15)]
    operands += [("SNARKV_QUOT_CONST(%d)" % i, Q.CONST(i)) for i in (0, 1, 1023)]
    operands += [("SNARKV_QUOT_COL(%d, %d)" % (c, rot), Q.COL(c, rot))
                 for c in (0, 1, (1 << 20) - 1) for rot in (-512, -1, 0, 1, 511)]
    consts = [("SNARKV_QUOT_REGS", Q.REGS), ("SNARKV_QUOT_ADD", Q.ADD), ("SNARKV_QUOT_SUB", Q.SUB), ("SNARKV_QUOT_MUL", Q.MUL),
              ("SNARKV_QUOT_FMA", Q.FMA), ("SNARKV_QUOT_MAX_INSTR", Q.MAX_INSTR), ("SNARKV_QUOT_MAX_CONSTS", Q.MAX_CONSTS),
              ("SNARKV_QUOT_MAX_COLS", Q.MAX_COLS), ("SNARKV_QUOT_MAX_E", Q.MAX_E), ("sizeof(snarkv_quot_instr)", Q.INSTR_BYTES)]
    exprs = operands + consts
    src = tmp_path / "words.c"
    src.write_text('#include <stdio.h>\n#include "snarkv_quotient.h"\nint main(void) {\n  snarkv_quot_instr i = {SNARKV_QUOT_FMA, 5, 0, '
                   'SNARKV_QUOT_REG(1), SNARKV_QUOT_CONST(2), SNARKV_QUOT_COL(3, -1)};\n'
                   '  fwrite(&i, sizeof i, 1, stdout);\n'
                   + "".join('  printf("\\n%%lu", (unsigned long)(%s));\n' % e for e, _ in exprs) + "  return 0;\n}\n")
    exe = tmp_path / "words"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, check=True).stdout
    assert out[:16] == Q.pack_instr(Q.FMA, 5, Q.REG(1), Q.CONST(2), Q.COL(3, -1))
    assert [int(v) for v in out[16:].split()] == [v for _, v in exprs]
    p = Q.Program()
    p.fma(5, p.mul(1, Q.COL(0), Q.COL(0)), p.const(9), Q.COL(3, -1))
    assert p.const(9) == Q.CONST(0) and p.const(4) == Q.CONST(1) and p.consts == [9, 4] and len(p) == 2
    assert p.packed() == Q.pack_instr(Q.MUL, 1, Q.COL(0), Q.COL(0)) + Q.pack_instr(Q.FMA, 5, Q.REG(1), Q.CONST(0), Q.COL(3, -1))


def test_every_refusal_comes_without_a_device():
    """(a correct call is never made here: a fake context must not reach the runtime)"""
    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt
    from snark_verifier_amd import quotient as Q

    ARG, ENC, EMPTY, LENGTH = sv.SNARKV_ERR_ARG, sv.SNARKV_ERR_ENCODING, sv.SNARKV_ERR_EMPTY, sv.SNARKV_ERR_LENGTH
    for pallas, curve in ((False, "bn254"), (True, "pallas")):
        a = Q.api(pallas)
        r = FIELD[curve]
        max_k = int(ntt.api(pallas).ntt_max_k())
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
        k, e, n_cols = 4, 2, 3
        n_ext = 1 << (k + e)
        col, ext = 32 << k, 32 << (k + e)
        # device addresses are only compared here, never followed
        COEFFS, COLS, OUT, WORK, H = ((1 << 44) * i for i in (1, 2, 3, 4, 5))
        assert n_ext * 32 == ext

        def overlap(rc):
            return rc == ARG and "overlap" in a.last_error()

        # ---- extend
        def ex(c=pc, i=COEFFS, kk=k, ee=e, cnt=n_cols, s=fe(5), o=OUT):
            return a.poly_extend_dev(c, i, kk, ee, cnt, s, o)

        assert ex(c=None) == ARG and ex(i=None) == ARG and ex(o=None) == ARG and ex(s=None) == ARG
        assert ex(i=COEFFS + 8) == ARG and ex(o=OUT + 4) == ARG  # 16-byte alignment
        assert ex(s=fe(0)) == ARG and "shift" in a.last_error()
        for o in (COEFFS, COEFFS + 32, COEFFS + n_cols * col - 32, COEFFS - n_cols * ext + 32):
            assert overlap(ex(o=o)), o - COEFFS
        assert ex(s=fe(r)) == ENC and ex(s=b"\xff" * 32) == ENC
        assert ex(cnt=0) == EMPTY
        assert ex(ee=9) == LENGTH and ex(kk=max_k, ee=1) == LENGTH and ex(kk=max_k + 1, ee=0) == LENGTH and ex(cnt=65536) == LENGTH
        # the order: arguments, then the encoding, then empty, then the lengths
        assert ex(i=None, s=fe(r)) == ARG and overlap(ex(o=COEFFS + 32, s=fe(r))) and ex(s=fe(0), cnt=0) == ARG
        assert ex(s=fe(r), cnt=0) == ENC and ex(s=fe(r), ee=9) == ENC and ex(cnt=0, ee=9) == EMPTY

        # ---- eval
        good = [(Q.MUL, 0, Q.COL(0), Q.COL(2, -1)), (Q.FMA, 1, Q.REG(0), Q.CONST(1), Q.COL(1, 511)), (Q.SUB, 1, Q.REG(1), Q.REG(0))]
        ok_c = fe(1) + fe(r - 1)

        def code(instrs):
            return b"".join(Q.pack_instr(*i) for i in instrs)

        def ev(c=pc, cols=COLS, kk=k, ee=e, nc=n_cols, prog=good, ni=None, cs=ok_c, ncs=2, o=OUT):
            packed = None if prog is None else (code(prog) if isinstance(prog, list) else prog)
            return a.quotient_eval_dev(c, cols, kk, ee, nc, packed, len(prog) if ni is None else ni, cs, ncs, o)

        assert ev(c=None) == ARG and ev(cols=None) == ARG and ev(o=None) == ARG and ev(prog=None, ni=3) == ARG and ev(cs=None) == ARG
        assert ev(cols=COLS + 8) == ARG and ev(o=OUT + 8) == ARG
        # every program fault on its own
        faults = {
            "read before write": [(Q.ADD, 0, Q.COL(0), Q.REG(2))],
            "read of itself before write": [(Q.MUL, 2, Q.REG(2), Q.COL(0))],
            "written only later": [(Q.ADD, 3, Q.REG(0), Q.REG(5)), (Q.ADD, 5, Q.REG(0), Q.REG(0))],
            "dst 16": [(Q.ADD, 16, Q.COL(0), Q.COL(1))],
            "register 16": [(Q.ADD, 1, Q.REG(16), Q.COL(1))],
            "kind 3": [(Q.ADD, 0, Q.COL(0), 3 << 30)],
            "kind 3 in c": [(Q.FMA, 0, Q.COL(0), Q.COL(0), (3 << 30) | 1)],
            "c on ADD": [(Q.ADD, 0, Q.COL(0), Q.COL(1), Q.COL(0))],
            "c on SUB": [(Q.SUB, 0, Q.COL(0), Q.COL(1), 1)],
            "c on MUL": [(Q.MUL, 0, Q.COL(0), Q.COL(1), Q.CONST(0))],
            "unknown op": [(4, 0, Q.COL(0), Q.COL(1))],
            "zero field": [(Q.ADD, 0, Q.COL(0), Q.COL(1), 0, 1)],
            "column = n_cols": [(Q.ADD, 0, Q.COL(0), Q.COL(n_cols))],
            "column = n_cols in c": [(Q.FMA, 0, Q.COL(0), Q.COL(1), Q.COL(n_cols, -3))],
            "constant = n_consts": [(Q.ADD, 0, Q.CONST(2), Q.COL(1))],
        }
        for name, bad in faults.items():
            assert ev(prog=good + bad) == ARG, name
            assert "instruction %d" % len(good) in a.last_error(), (name, a.last_error())
        for o in (COLS, COLS + 32, COLS + n_cols * ext - 32, COLS - ext + 32):  # out in any part of the columns
            assert overlap(ev(o=o)), o - COLS
        assert ev(cs=fe(1) + fe(r)) == ENC and ev(cs=b"\xff" * 32 + fe(2)) == ENC
        assert ev(nc=0) == EMPTY and ev(ni=0) == EMPTY
        many = [(Q.ADD, 0, Q.COL(0), Q.COL(1))] * 4097
        assert ev(prog=many) == LENGTH and ev(prog=many[:4096], ee=9) == LENGTH
        assert ev(cs=fe(1) * 1025, ncs=1025) == LENGTH and ev(nc=(1 << 20) + 1, o=(1 << 62)) == LENGTH
        assert ev(ee=9) == LENGTH and ev(kk=max_k - 1) == LENGTH
        # the order
        assert ev(prog=good + faults["kind 3"], cs=fe(r) * 2) == ARG and overlap(ev(o=COLS, cs=fe(r) * 2))
        assert ev(cs=fe(r) * 2, nc=0) == ENC and ev(cs=fe(r) * 2, prog=many) == ENC and ev(nc=0, ee=9) == EMPTY
        assert ev(prog=many + faults["dst 16"]) == ARG and ev(cols=None, ni=0) == ARG

        # ---- div_vanishing
        def dv(c=pc, i=COLS, kk=k, ee=e, s=fe(5), o=OUT):
            return a.poly_div_vanishing_dev(c, i, kk, ee, s, o)

        assert dv(c=None) == ARG and dv(i=None) == ARG and dv(o=None) == ARG and dv(s=None) == ARG and dv(i=COLS + 8) == ARG
        assert dv(o=OUT + 8) == ARG and dv(s=fe(0)) == ARG
        for o in (COLS + 32, COLS - 32, COLS + ext - 32, COLS - ext + 32):
            assert overlap(dv(o=o)), o - COLS
        assert dv(s=fe(r)) == ENC and dv(ee=9) == LENGTH and dv(kk=max_k, ee=1) == LENGTH
        assert dv(o=COLS, ee=9) == LENGTH  # in place is allowed, so it reaches the length check
        assert overlap(dv(o=COLS + 32, s=fe(r))) and dv(s=fe(r), ee=9) == ENC

        # ---- quotient
        def qd(c=pc, i=COEFFS, kk=k, ee=e, nc=n_cols, prog=good, ni=None, cs=ok_c, ncs=2, s=fe(5), si=fe(7), w=WORK, h=H):
            packed = None if prog is None else code(prog)
            return a.quotient_dev(c, i, kk, ee, nc, packed, len(prog) if ni is None else ni, cs, ncs, s, si, w, h)

        assert qd(c=None) == ARG and qd(i=None) == ARG and qd(w=None) == ARG and qd(h=None) == ARG and qd(prog=None, ni=1) == ARG
        assert qd(cs=None) == ARG and qd(s=None) == ARG and qd(si=None) == ARG and qd(s=fe(0)) == ARG and qd(si=fe(0)) == ARG
        assert qd(i=COEFFS + 8) == ARG and qd(w=WORK + 8) == ARG and qd(h=H + 4) == ARG
        for name, bad in faults.items():
            assert qd(prog=good + bad) == ARG, name
        # work (n_cols extended columns), h (one) and the coefficients: pairwise disjoint
        assert overlap(qd(h=WORK)) and overlap(qd(h=WORK + n_cols * ext - 32)) and overlap(qd(h=WORK - ext + 32))
        assert overlap(qd(w=COEFFS + n_cols * col - 32)) and overlap(qd(w=COEFFS - n_cols * ext + 32))
        assert overlap(qd(h=COEFFS + 32)) and overlap(qd(h=COEFFS - ext + 32))
        assert qd(cs=fe(r) * 2) == ENC and qd(s=fe(r)) == ENC and qd(si=fe(r + 1)) == ENC
        assert qd(nc=0) == EMPTY and qd(ni=0) == EMPTY
        assert qd(prog=many) == LENGTH and qd(ee=9) == LENGTH and qd(kk=max_k - 1) == LENGTH
        assert qd(cs=fe(1) * 1025, ncs=1025) == LENGTH and qd(nc=(1 << 20) + 1, w=(1 << 61), h=(1 << 58)) == LENGTH
        assert qd(prog=good + faults["kind 3"], s=fe(r)) == ARG and overlap(qd(h=WORK, si=fe(r)))
        assert qd(si=fe(r), nc=0) == ENC and qd(si=fe(r), ee=9) == ENC and qd(nc=0, ee=9) == EMPTY
