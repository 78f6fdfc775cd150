"""Shared helpers of the tests of the transform over group elements (include/snarkv_g1_ntt.h): the reference, a plain
radix-2 transform (bit reversal, then log2(n) levels of butterflies) on the oracle's point arithmetic with the domain generator
of tests/ntt_util.py, the O(n^2) sums of the header for small n, the special inputs, and byte packing."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ntt_util as NU  # noqa: E402

CURVES = NU.CURVES
FORWARD, INVERSE = NU.FORWARD, NU.INVERSE


def _jdbl(P, p):
    x, y, z = p
    if z == 0 or y == 0:
        return (1, 1, 0)
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return (x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P)


def _jmadd(P, p, q):
    """p (Jacobian) + q (affine, not the identity)"""
    if p[2] == 0:
        return (q[0], q[1], 1)
    zz = p[2] * p[2] % P
    u2, s2 = q[0] * zz % P, q[1] * p[2] * zz % P
    if u2 == p[0]:
        return _jdbl(P, p) if s2 == p[1] else (1, 1, 0)
    h, r = (u2 - p[0]) % P, (s2 - p[1]) % P
    hh = h * h % P
    hhh, v = h * hh % P, p[0] * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - p[1] * hhh) % P, p[2] * h % P)


def mul(O, p, e):
    """e * p, e taken mod r: left-to-right double-and-add in Jacobian coordinates (j = 0 curves), one inversion.  The
    oracle's BN254 g1_mul inverts at every step; tests/test_g1_ntt_host.py holds this one against it."""
    e %= O.R
    if p is None or e == 0:
        return None
    if 2 * e > O.R:  # half the additions for the small negative powers
        p, e = O.g1_neg(p), O.R - e
    acc = (1, 1, 0)
    for bit in bin(e)[2:]:
        acc = _jdbl(O.P, acc)
        if bit == "1":
            acc = _jmadd(O.P, acc, p)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, O.P)
    return (acc[0] * zi * zi % O.P, acc[1] * zi * zi * zi % O.P)


_mul = mul


def reference(curve, pts, direction):
    """what snarkv_g1_ntt_dev computes: out[i] = sum_j w^(ij) pts[j], or n^-1 sum_j w^(-ij) pts[j]; None is the identity"""
    O = CURVES[curve]
    n = len(pts)
    k = n.bit_length() - 1
    assert n == 1 << k
    w = NU.omega(curve, k)
    if direction == INVERSE:
        w = pow(w, -1, O.R)
    a = [pts[int(format(i, "0%db" % k)[::-1], 2)] if k else pts[i] for i in range(n)]
    half = 1
    while half < n:
        step = pow(w, n // (2 * half), O.R)
        tw = [pow(step, i, O.R) for i in range(half)]
        for base in range(0, n, 2 * half):
            for i in range(half):
                u, t = a[base + i], (a[base + half + i] if i == 0 else _mul(O, a[base + half + i], tw[i]))
                a[base + i], a[base + half + i] = O.g1_add(u, t), O.g1_add(u, O.g1_neg(t))
        half *= 2
    if direction == INVERSE and k:
        n_inv = pow(n, -1, O.R)
        a = [_mul(O, p, n_inv) for p in a]
    return a


def definition(curve, pts, direction):
    """the O(n^2) sums of the header, for small n"""
    O = CURVES[curve]
    n = len(pts)
    w = NU.omega(curve, n.bit_length() - 1)
    if direction == INVERSE:
        w = pow(w, -1, O.R)
    scale = pow(n, -1, O.R) if direction == INVERSE else 1
    out = []
    for i in range(n):
        acc = None
        for j in range(n):
            acc = O.g1_add(acc, _mul(O, pts[j], pow(w, i * j, O.R) * scale))
        out.append(acc)
    return out


def random_points(curve, n, tag=""):
    """n multiples of the generator by random scalars"""
    O = CURVES[curve]
    rnd = random.Random("g1-ntt-%s-%s" % (curve, tag))
    return [O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R)) for _ in range(n)]


def special_inputs(curve, n):
    """name -> n points: what makes the additions of a butterfly exceptional"""
    O = CURVES[curve]
    p, q = random_points(curve, 2, "special")
    with_ids = random_points(curve, n, "ids")
    for i in range(0, n, 3):
        with_ids[i] = None
    return {
        "equal": [p] * n,  # every difference is the identity, every sum a doubling
        "alternating": [p if i % 2 == 0 else O.g1_neg(p) for i in range(n)],
        "identities": with_ids,
        "all-identities": [None] * n,
        "one-point": [q] + [None] * (n - 1),  # every later a + t has a = t or t = identity
    }


def pack(curve, pts):
    O = CURVES[curve]
    return b"".join(O.g1_to_bytes(p) for p in pts)


def unpack(curve, raw):
    O = CURVES[curve]
    return [O.g1_from_bytes(raw[i:i + 64]) for i in range(0, len(raw), 64)]
