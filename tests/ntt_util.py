"""Shared helpers of the transform tests: the reference (a short iterative radix-2 transform over Python integers, with the
domain generator of oracle/plonk.py::root_of_unity), Horner evaluation, and byte packing."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402
import plonk as PK  # noqa: E402

CURVES = {"bn254": BN, "pallas": PA}
FORWARD, INVERSE = 0, 1


_OMEGA = {}


def omega(curve, k):
    """root_of_unity(k) of the curve's scalar field.  The oracle stack is switched to the curve for the call and back to BN254,
    its default, afterwards: a test that has switched it itself does so again after calling this."""
    if (curve, k) not in _OMEGA:
        PK.use_curve(CURVES[curve])
        try:
            _OMEGA[(curve, k)] = PK.root_of_unity(k)
        finally:
            PK.use_curve(BN)
    return _OMEGA[(curve, k)]


def _radix2(a, w, r):
    """sum_j a[j] w^(i j), natural order in and out: bit reversal, then log2(n) levels of butterflies"""
    n = len(a)
    k = n.bit_length() - 1
    a = [a[int(format(i, "0%db" % k)[::-1], 2)] if k else a[i] for i in range(n)]
    half = 1
    while half < n:
        step = pow(w, n // (2 * half), r)
        tw = [1] * half
        for i in range(1, half):
            tw[i] = tw[i - 1] * step % r
        for base in range(0, n, 2 * half):
            for i in range(half):
                u, t = a[base + i], a[base + half + i] * tw[i] % r
                a[base + i], a[base + half + i] = (u + t) % r, (u - t) % r
        half *= 2
    return a


def reference(curve, vals, direction, shift=None):
    """what snarkv_ntt_dev computes (include/snarkv_ntt.h) for one polynomial"""
    r = CURVES[curve].R
    n = len(vals)
    k = n.bit_length() - 1
    w, s = omega(curve, k), 1 if shift is None else shift
    if direction == FORWARD:
        a, p = [], 1
        for v in vals:
            a.append(v * p % r)
            p = p * s % r
        return _radix2(a, w, r)
    out, p, n_inv = [], pow(n, -1, r), 1
    for v in _radix2(list(vals), pow(w, -1, r), r):
        out.append(v * p % r * n_inv % r)
        n_inv = n_inv * s % r
    return out


def definition(curve, vals, direction, shift=None):
    """the O(n^2) sums of the header, for small n"""
    r = CURVES[curve].R
    n = len(vals)
    w, s = omega(curve, n.bit_length() - 1), 1 if shift is None else shift
    if direction == FORWARD:
        return [sum(pow(s, j, r) * vals[j] * pow(w, i * j, r) for j in range(n)) % r for i in range(n)]
    wi = pow(w, -1, r)
    return [pow(s, j, r) * pow(n, -1, r) * sum(vals[i] * pow(wi, i * j, r) for i in range(n)) % r for j in range(n)]


def horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
