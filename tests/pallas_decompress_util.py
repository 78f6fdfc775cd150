"""Shared by the CPU and GPU tests of the pallas point decompression: what `pallas::Affine::from_bytes` answers, from
the oracle's square root (oracle/pallas.py::fq_sqrt), and seeded inputs with a known 2-adic order of x^3 + 5."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import pallas as PA  # noqa: E402

P = PA.P
S = 32
T = (P - 1) >> S
assert T % 2 == 1 and T << S == P - 1


def order_exponent(a):
    """i with a^t of order exactly 2^i (a != 0): 32 for a non-square, at most 31 for a square."""
    b, i = pow(a, T, P), 0
    while b != 1:
        b, i = b * b % P, i + 1
    return i


def encode(x, parity):
    return (x | (parity << 255)).to_bytes(32, "little")


def expected(enc, mont=False):
    """(64 bytes, ok) for one 32-byte encoding."""
    v = int.from_bytes(enc, "little")
    if v == 0:
        return bytes(64), 1
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x >= P:
        return bytes(64), 0
    y = PA.fq_sqrt(x * x * x + 5)
    if y is None:
        return bytes(64), 0
    if (y & 1) != sign and y != 0:
        y = P - y
    if mont:
        x, y = (x << 256) % P, (y << 256) % P
    return x.to_bytes(32, "little") + y.to_bytes(32, "little"), 1


def seeded_pairs(seed, n):
    rnd = random.Random(seed)
    return [(rnd.randrange(P), rnd.getrandbits(1)) for _ in range(n)]
