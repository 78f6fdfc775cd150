"""CPU: the coset-at-a-time route to the quotient (include/snarkv_quotient_cosets.h) on Python integers
(tests/quotient_cosets_util.py) against the reference of tests/quotient_util.py, and the join's SNARKV_HD text
(snark-verifier_amd/csrc/quotient.h) run on the host through tests/hosttest/hosttest_quotient_cosets.cpp for both curves
against those integers: every (k, e) in 0..4 x 0..3 and (1, 8), (2, 8); the shift zeta, the shift 1 and a shift W for which a
vanishing entry is zero (the zero rule); random programs and the small circuit; every input word r - 1 and input words >= r;
in place and out of place.  Every comparison is on whole lists of canonical values, nothing is filtered."""
import ctypes
import importlib.util
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quotient_cosets_util as CU  # noqa: E402
import quotient_util as QU  # noqa: E402

CURVES = ["bn254", "pallas"]
SHAPES = CU.MODEL_SHAPES
_LIBS = {}


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("quotient_cosets", curve))
        lib.hqc_curve.restype = ctypes.c_char_p
        lib.hqc_tile_bits.restype = ctypes.c_uint32
        lib.hqc_join.restype = None
        lib.hqc_coset_shifts.restype = None
        assert lib.hqc_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


@pytest.fixture(scope="module")
def Q():
    from snark_verifier_amd import quotient

    return quotient


def _words(vals):
    raw = QU.pack(vals)
    return (ctypes.c_uint32 * (len(raw) // 4)).from_buffer_copy(raw)


def host_join(curve, rows, k, e, shift_inv, factors=None, in_place=False):
    lib, n_ext = host_lib(curve), 1 << (k + e)
    src = _words(sum(rows, []))
    out = src if in_place else (ctypes.c_uint32 * (8 * n_ext))(*([0xAAAAAAAA] * (8 * n_ext)))
    lib.hqc_join(src, k, e, _words([shift_inv]), None if factors is None else _words(factors), out)
    return QU.unpack(bytes(out))


# ---------------------------------------------------------------- the route on integers
@pytest.mark.parametrize("curve", CURVES)
def test_the_cosets_are_the_rows_of_the_extended_coset(curve):
    rnd = random.Random("quotient-cosets-rows-" + curve)
    r = QU.FIELD[curve]
    for k, e in SHAPES:
        f = [rnd.randrange(r) for _ in range(1 << k)]
        for s in (QU.zeta(curve), 1):
            rows = [CU.coset_values(curve, f, k, e, s, j) for j in range(1 << e)]
            assert CU.interleave(rows) == QU.extend(curve, f, k, e, s), (k, e, s)


@pytest.mark.parametrize("curve", CURVES)
def test_the_join_alone_is_the_large_inverse_transform(curve):
    rnd = random.Random("quotient-cosets-join-" + curve)
    r = QU.FIELD[curve]
    for k, e in SHAPES:
        rows = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(1 << e)]
        for s in (QU.zeta(curve), 1, rnd.randrange(1, r)):
            s_inv = pow(s, -1, r)
            assert CU.join_values(curve, rows, k, e, s_inv) == QU.to_coeffs(curve, CU.interleave(rows), s_inv), (k, e, s)


@pytest.mark.parametrize("curve", CURVES)
def test_random_programs_by_cosets(Q, curve):
    r = QU.FIELD[curve]
    for k, e in SHAPES:
        rnd = random.Random("quotient-cosets-model-%s-%d-%d" % (curve, k, e))
        n_cols, n_consts = 3, 4
        instrs = QU.random_program(Q, rnd, 24 if e < 8 else 6, n_cols, n_consts)
        coeffs = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(n_cols)]
        consts = [rnd.randrange(r) for _ in range(n_consts)]
        shifts = (QU.zeta(curve), 1) if e < 8 else (QU.zeta(curve),)
        for s in shifts:
            assert CU.quotient_by_cosets(curve, coeffs, k, e, instrs, consts, s) == QU.quotient(curve, coeffs, k, e, instrs, consts, s), (k, e, s)


@pytest.mark.parametrize("curve", CURVES)
def test_the_zero_rule(Q, curve):
    """s = 1 makes entry 0 of the vanishing table zero, s = W entry 2^e - 1: the coset counts as zero on both routes"""
    r = QU.FIELD[curve]
    rnd = random.Random("quotient-cosets-zero-" + curve)
    for k, e in ((0, 0), (0, 3), (1, 1), (3, 2), (2, 3), (1, 4)):
        instrs = QU.random_program(Q, rnd, 12, 2, 2)
        coeffs = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(2)]
        consts = [rnd.randrange(r) for _ in range(2)]
        for s, at in ((1, 0), (CU.root_shift(curve, k, e), (1 << e) - 1)):
            assert QU.vanishing_table(curve, k, e, s)[at] == 0
            assert CU.quotient_by_cosets(curve, coeffs, k, e, instrs, consts, s) == QU.quotient(curve, coeffs, k, e, instrs, consts, s), (k, e, s)


@pytest.mark.parametrize("bad", [None, "gate", "copy"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_small_circuit_by_cosets(Q, curve, bad):
    k, e = 4, 2
    c = QU.Circuit(curve, k, bad)
    coeffs = c.coeff_columns(c.z()[0])
    p = c.program(Q)
    h = CU.quotient_by_cosets(curve, coeffs, k, e, p.instrs, p.consts, QU.zeta(curve))
    assert h == QU.quotient(curve, coeffs, k, e, p.instrs, p.consts, QU.zeta(curve))
    assert all(v == 0 for v in h[3 * (1 << k) - 3:]) == (bad is None)
    # the shift 1: a coset is dropped, both routes drop the same one
    assert CU.quotient_by_cosets(curve, coeffs, k, e, p.instrs, p.consts, 1) == QU.quotient(curve, coeffs, k, e, p.instrs, p.consts, 1)


# ---------------------------------------------------------------- the device's text on the host
@pytest.mark.parametrize("curve", CURVES)
def test_host_join_against_the_integers(curve):
    r = QU.FIELD[curve]
    for k, e in SHAPES:
        rnd = random.Random("quotient-cosets-host-%s-%d-%d" % (curve, k, e))
        n, m = 1 << k, 1 << e
        assert host_lib(curve).hqc_tile_bits(k, e) == min(k, 10 - e)
        inputs = {
            "random": [[rnd.randrange(r) for _ in range(n)] for _ in range(m)],
            "all r-1": [[r - 1] * n for _ in range(m)],
            "words >= r": [[rnd.choice([r, r + 1, (1 << 256) - 1, rnd.randrange(r, 1 << 256)]) for _ in range(n)] for _ in range(m)],
        }
        factors = [rnd.choice([0, 1, r - 1, rnd.randrange(r)]) for _ in range(m)]
        for name, rows in inputs.items():
            for s_inv in (pow(QU.zeta(curve), -1, r), 1, r - 1):
                want = CU.join(curve, rows, k, e, s_inv)
                assert host_join(curve, rows, k, e, s_inv) == want, (k, e, name, s_inv)
                assert host_join(curve, rows, k, e, s_inv, in_place=True) == want, (k, e, name, "in place")
            s_inv = rnd.randrange(1, r)
            assert host_join(curve, rows, k, e, s_inv, factors) == CU.join(curve, rows, k, e, s_inv, factors), (k, e, name, "factors")


@pytest.mark.parametrize("curve", CURVES)
def test_host_join_past_one_tile(curve):
    """n larger than the tile: k = 9 at e = 2 (two tiles of 256 t), k = 4 at e = 8 (four tiles of 4 t), and every level of the
    exponent tables at k + e = 12 > 8"""
    r = QU.FIELD[curve]
    for k, e in ((9, 2), (4, 8), (11, 0)):
        rnd = random.Random("quotient-cosets-tiles-%s-%d-%d" % (curve, k, e))
        rows = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(1 << e)]
        s_inv = pow(QU.zeta(curve), -1, r)
        assert host_lib(curve).hqc_tile_bits(k, e) < k
        got = host_join(curve, rows, k, e, s_inv, in_place=True)
        # against the large inverse transform: the join after the size-k inverse transforms
        vals = [QU.U.reference(curve, row, QU.U.FORWARD) for row in rows]
        assert got == QU.to_coeffs(curve, CU.interleave(vals), s_inv), (k, e)


@pytest.mark.parametrize("curve", CURVES)
def test_host_coset_shifts(curve):
    r, lib = QU.FIELD[curve], host_lib(curve)
    for k, e in SHAPES:
        for s in (QU.zeta(curve), 1, r - 1):
            out = (ctypes.c_uint32 * (8 << e))()
            lib.hqc_coset_shifts(_words([s]), k, e, out)
            assert QU.unpack(bytes(out)) == CU.coset_shifts(curve, k, e, s), (k, e, s)
