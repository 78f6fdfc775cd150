"""CPU: the blocked scan behind `poly_div_linear_dev` and `poly_eval_dev` (snark-verifier_amd/csrc/poly_scan.h, the source
the device compiles), run on the host through tests/hosttest/hosttest_poly.cpp for both curves with blocks of 2, 3 and 4
coefficients, against Python integers: the quotient and remainder of the recurrence c_i = p_i + a c_{i+1}, the identity
p = (X - a) quot + rem coefficient by coefficient, and p(a) from the totals alone."""
import ctypes
import importlib.util
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

CURVES = {"bn254": BN.R, "pallas": PA.R}
LENGTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65]


def host_lib(curve):
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lib = ctypes.CDLL(b.build_hosttest("poly", curve))
    lib.hp_curve.restype = ctypes.c_char_p
    lib.hp_query_sets.restype = ctypes.c_size_t
    assert lib.hp_curve() == curve.encode()
    return lib


def _words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).copy()


def _ints(arr):
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def div_linear(p, a, r):
    """oracle/ipa.py::_poly_div_linear with the remainder kept"""
    out, carry = [0] * (len(p) - 1), 0
    for i in range(len(p) - 1, 0, -1):
        carry = (p[i] + carry * a) % r
        out[i - 1] = carry
    return out, (p[0] + carry * a) % r


def _run(lib, p, a, block):
    n, vp = len(p), ctypes.c_void_p
    quot, rem, val = np.zeros(8 * max(n - 1, 1), dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
    assert lib.hp_div_linear(_words(p).ctypes.data_as(vp), n, _words([a]).ctypes.data_as(vp), block, quot.ctypes.data_as(vp),
                             rem.ctypes.data_as(vp), val.ctypes.data_as(vp)) == 1
    return _ints(quot)[:n - 1], _ints(rem)[0], _ints(val)[0]


@pytest.mark.parametrize("block", [2, 3, 4])
@pytest.mark.parametrize("curve", sorted(CURVES))
def test_quotient_remainder_and_value(curve, block):
    r, lib = CURVES[curve], host_lib(curve)
    rnd = random.Random("poly-scan-%s-%d" % (curve, block))
    for n in LENGTHS:
        shapes = [[rnd.randrange(r) for _ in range(n)], [r - 1] * n]
        for a in (0, 1, r - 1, rnd.randrange(r)):
            for p in shapes:
                quot, rem, val = _run(lib, p, a, block)
                want_q, want_r = div_linear(p, a, r)
                assert (quot, rem) == (want_q, want_r), (n, a)
                assert val == want_r  # the same source evaluates p(a)
                # p == (X - a) quot + rem, coefficient by coefficient
                q = quot + [0]
                assert p[0] == (rem - a * q[0]) % r
                for i in range(1, n):
                    assert p[i] == (q[i - 1] - a * q[i]) % r, (n, a, i)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_exact_multiple_and_off_by_one(curve):
    r, lib = CURVES[curve], host_lib(curve)
    rnd = random.Random("poly-scan-exact-" + curve)
    for n in (2, 5, 17, 65):
        a = rnd.randrange(r)
        q = [rnd.randrange(r) for _ in range(n - 1)]
        p = [(x - a * y) % r for x, y in zip([0] + q, q + [0])]  # (X - a) q
        assert _run(lib, p, a, 4) == (q, 0, 0)
        p[0] = (p[0] + 1) % r
        assert _run(lib, p, a, 3) == (q, 1, 1)
