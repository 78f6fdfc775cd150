"""CPU: the quotient's gate program and vanishing table (snark-verifier_amd/csrc/quotient.h, the source the device compiles),
run on the host through tests/hosttest/hosttest_quotient.cpp for both curves against Python integers (tests/quotient_util.py):
random programs of 1 to 200 instructions over all four ops at every (k, e) in 0..4 x 0..3, with all 16 registers used, a
destination that is one of its sources, and the rotations -512, -1, 0, 1, 511; every operand r - 1; column words >= r; the
row a rotation reads; the vanishing table at every (k, e); and the small circuit end to end on integers, the CPU statement of
what tests/test_gpu_quotient.py checks.  Every comparison is on canonical words, nothing is filtered."""
import ctypes
import importlib.util
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quotient_util as QU  # noqa: E402

CURVES = ["bn254", "pallas"]
SHAPES = [(k, e) for k in range(5) for e in range(4)]
_LIBS = {}


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("quotient", curve))
        lib.hq_curve.restype = ctypes.c_char_p
        lib.hq_two_adicity.restype = ctypes.c_uint32
        lib.hq_row.restype = ctypes.c_uint32
        lib.hq_eval.restype = None
        lib.hq_vanishing_table.restype = None
        assert lib.hq_curve() == curve.encode()
        assert lib.hq_two_adicity() == QU.GENERATOR[curve][1]
        _LIBS[curve] = lib
    return _LIBS[curve]


@pytest.fixture(scope="module")
def Q():
    from snark_verifier_amd import quotient

    return quotient


def _words(vals):
    raw = QU.pack(vals) or b"\x00" * 32
    return (ctypes.c_uint32 * (len(raw) // 4)).from_buffer_copy(raw)


def host_eval(Q, curve, cols, k, e, instrs, consts):
    lib, n_ext = host_lib(curve), 1 << (k + e)
    out = (ctypes.c_uint32 * (8 * n_ext))(*([0xAAAAAAAA] * (8 * n_ext)))
    code = QU.pack_program(Q, instrs)
    lib.hq_eval(_words(sum(cols, [])), k, e, code, len(instrs), _words(consts), len(consts), out)
    return QU.unpack(bytes(out))


@pytest.mark.parametrize("curve", CURVES)
def test_random_programs(Q, curve):
    r = QU.FIELD[curve]
    lengths = [1, 2, 3, 16, 17, 64, 200]
    for at, (k, e) in enumerate(SHAPES):
        rnd = random.Random("quotient-model-%s-%d-%d" % (curve, k, e))
        n_ext, n_cols, n_consts = 1 << (k + e), 3, 4
        for n_instr in (lengths[at % len(lengths)], lengths[(at + 3) % len(lengths)]):
            instrs = QU.random_program(Q, rnd, n_instr, n_cols, n_consts)
            assert QU.decode(QU.pack_program(Q, instrs)) == instrs
            if n_instr >= 64:
                assert {i[1] for i in instrs} == set(range(16))
                assert any(Q.REG(i[1]) in i[2:4] for i in instrs), "a destination that is a source"
            inputs = {
                "random": ([[rnd.randrange(r) for _ in range(n_ext)] for _ in range(n_cols)], [rnd.randrange(r) for _ in range(n_consts)]),
                "all r-1": ([[r - 1] * n_ext for _ in range(n_cols)], [r - 1] * n_consts),
                "words >= r": ([[rnd.choice([r, r + 1, (1 << 256) - 1, rnd.randrange(r, 1 << 256)]) for _ in range(n_ext)]
                                for _ in range(n_cols)], [rnd.choice([0, 1, r - 1]) for _ in range(n_consts)]),
            }
            for name, (cols, consts) in inputs.items():
                got = host_eval(Q, curve, cols, k, e, instrs, consts)
                assert got == QU.interpret(curve, cols, k, e, instrs, consts), (k, e, n_instr, name)


@pytest.mark.parametrize("curve", CURVES)
def test_each_op_with_every_operand_r_minus_1(Q, curve):
    """the largest sums the bounds of quotient.h meet: (r-1) + (r-1), 0 - (r-1), (r-1)(r-1) + (r-1), and chains of them
    through registers, where a sum is an operand of the next sum and of the next product"""
    r = QU.FIELD[curve]
    for edge in (r - 1, 0, 1):
        cols, consts = [[edge] * 2], [r - 1, 0]
        c0, k0, k1 = Q.COL(0), Q.CONST(0), Q.CONST(1)
        programs = [[(op, 0, c0, k0, k0 if op == QU.FMA else 0)] for op in (QU.ADD, QU.SUB, QU.MUL, QU.FMA)]
        programs.append([(QU.SUB, 0, k1, c0, 0), (QU.SUB, 1, k1, k0, 0), (QU.SUB, 2, Q.REG(0), k0, 0), (QU.ADD, 3, Q.REG(2), Q.REG(2), 0),
                         (QU.FMA, 4, Q.REG(3), Q.REG(3), Q.REG(3)), (QU.SUB, 4, Q.REG(1), Q.REG(4), 0), (QU.MUL, 4, Q.REG(4), Q.REG(4), 0),
                         (QU.FMA, 0, Q.REG(4), k0, k0)])
        programs.append([(QU.ADD, 0, k0, k0, 0)] + [(QU.ADD, 0, Q.REG(0), k0, 0), (QU.SUB, 0, k1, Q.REG(0), 0),
                                                     (QU.FMA, 0, Q.REG(0), Q.REG(0), Q.REG(0))] * 20)
        for instrs in programs:
            assert host_eval(Q, curve, cols, 0, 1, instrs, consts) == QU.interpret(curve, cols, 0, 1, instrs, consts), instrs


@pytest.mark.parametrize("curve", CURVES)
def test_the_row_of_a_rotation(Q, curve):
    lib = host_lib(curve)
    for k, e in SHAPES:
        n_ext = 1 << (k + e)
        for rot in QU.ROTATIONS + [2, -2, 255, -256]:
            word = Q.COL(7, rot)
            for row in {0, 1, n_ext // 2, n_ext - 1} & set(range(n_ext)):
                assert lib.hq_row(row, word, e, k + e) == QU.row_of(row, rot, e, n_ext), (k, e, rot, row)


@pytest.mark.parametrize("curve", CURVES)
def test_vanishing_table(curve):
    r, lib = QU.FIELD[curve], host_lib(curve)
    rnd = random.Random("quotient-model-vanishing-" + curve)
    for k, e in SHAPES:
        w_ext, n = QU.U.omega(curve, k + e), 1 << k
        for shift in (QU.zeta(curve), 1, r - 1, rnd.randrange(1, r)):
            out = (ctypes.c_uint32 * (8 << e))()
            lib.hq_vanishing_table(_words([shift]), k, e, out)
            got = QU.unpack(bytes(out))
            assert got == QU.vanishing_table(curve, k, e, shift), (k, e, shift)
            for i in range(1 << (k + e)):  # the definition, row by row
                assert got[i % (1 << e)] == (pow(shift * pow(w_ext, i, r), n, r) - 1) % r


@pytest.mark.parametrize("bad", [None, "gate", "copy"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_small_circuit_on_integers(Q, curve, bad):
    """k = 4, e = 2: the satisfied witness gives total = 1, the identity h(x)(x^n - 1) = expr(x) and zero coefficients from
    3n - 3 upward; each broken one fails the identity and the degree bound.  The host model gives the integers' values."""
    r, k, e = QU.FIELD[curve], 4, 2
    n, s = 1 << k, QU.zeta(curve)
    c = QU.Circuit(curve, k, bad)
    z, total = c.z()
    assert (total == 1) == (bad != "copy")
    coeffs = c.coeff_columns(z)
    p = c.program(Q)
    h = QU.quotient(curve, coeffs, k, e, p.instrs, p.consts, s)
    ext = [QU.extend(curve, col, k, e, s) for col in coeffs]
    assert host_eval(Q, curve, ext, k, e, p.instrs, p.consts) == QU.interpret(curve, ext, k, e, p.instrs, p.consts)
    x = random.Random("quotient-model-point-" + curve).randrange(r)
    ok, top = QU.identity_holds(c, coeffs, h, x), all(v == 0 for v in h[3 * n - 3:])
    assert ok == top == (bad is None)
    if bad is None:  # the gate alone at e = 1: degree 3, h below 2n
        g = c.program(Q, permutation=False)
        hg = QU.quotient(curve, coeffs, k, 1, g.instrs, g.consts, s)
        assert QU.identity_holds(c, coeffs, hg, x, permutation=False) and all(v == 0 for v in hg[2 * n - 2:])
