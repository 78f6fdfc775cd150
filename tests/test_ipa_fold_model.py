"""CPU: the fold kernel's per-lane body and partial sum (snark-verifier_amd/csrc/ipa_fold.h, the source the device compiles),
run on the host through tests/hosttest/hosttest_fold.cpp for both curves, against the big-integer definition
    h[j] = sum_{i<m} rho^i prod over the set bits b of j of xi_i[k-1-b]   (mod r)
for keys below, at and above a lane's block of 2^3 coefficients and every slice count 1..m."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

CURVES = {"bn254": BN.R, "pallas": PA.R}


def fold_definition(xis, rho, r):
    """sum rho^i h_coeffs(xi_i) in exact integers: h_coeffs by the doubling of pcs/ipa.rs:405-421"""
    k = len(xis[0])
    out, w = [0] * (1 << k), 1
    for xi in xis:
        h = [1]
        for x in reversed(xi):
            h = h + [c * x % r for c in h]
        out = [(o + w * c) % r for o, c in zip(out, h)]
        w = w * rho % r
    return out


def _host_lib(curve):
    """tests/hosttest/hosttest_fold.cpp compiled with g++ for one curve, rebuilt when stale"""
    d = os.path.join(ROOT, "tests", "hosttest")
    src, so = os.path.join(d, "hosttest_fold.cpp"), os.path.join(d, "libhosttest_fold_%s.so" % curve)
    csrc = os.path.join(ROOT, "snark-verifier_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        flags = ["-DSNARKV_CURVE_PALLAS"] if curve == "pallas" else []
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hf_curve.restype = ctypes.c_char_p
    assert lib.hf_curve() == curve.encode()
    return lib


def _words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).copy()


def _run(lib, xis, rho, slices):
    m, k = len(xis), len(xis[0])
    xi, rw = _words([x for xi in xis for x in xi]), _words([rho])
    h = np.zeros(8 << k, dtype=np.uint32)
    vp = ctypes.c_void_p
    lib.hf_fold_coeffs(xi.ctypes.data_as(vp), rw.ctypes.data_as(vp), m, k, slices, h.ctypes.data_as(vp))
    raw = h.tobytes()
    return [int.from_bytes(raw[32 * j:32 * j + 32], "little") for j in range(1 << k)]


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 9])
def test_lane_body_and_partial_sum_equal_the_definition(curve, k):
    r = CURVES[curve]
    lib = _host_lib(curve)
    from snark_verifier_amd import ipa_fold

    assert lib.hf_fold_block_bits() == ipa_fold.FOLD_BLOCK_BITS == 3
    rnd = random.Random("fold-model-%s-%d" % (curve, k))
    for m in (1, 2, 7):
        xis = [[rnd.randrange(r) for _ in range(k)] for _ in range(m)]
        if m == 7:
            xis[2] = [0] * k            # h_coeffs = (1, 0, 0, ...)
            xis[5] = [r - 1] * k        # every coefficient +-1
        for rho in (rnd.randrange(r), 0, 1, r - 1):
            want = fold_definition(xis, rho, r)
            for slices in range(1, m + 1):
                assert _run(lib, xis, rho, slices) == want, (curve, k, m, rho, slices)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_long_slices_pass_through_the_lazy_reduction(curve):
    """more than 32 accumulators per slice and more than 32 slices: the running sums are reduced on the way (every
    32 additions), with the extreme operands r - 1 throughout"""
    r = CURVES[curve]
    lib = _host_lib(curve)
    rnd = random.Random("fold-long-" + curve)
    k, m = 4, 70
    for xis, rho in (([[r - 1] * k for _ in range(m)], r - 1), ([[rnd.randrange(r) for _ in range(k)] for _ in range(m)], rnd.randrange(r))):
        want = fold_definition(xis, rho, r)
        for slices in (1, 2, 33, 70):
            assert _run(lib, xis, rho, slices) == want, (curve, slices)
