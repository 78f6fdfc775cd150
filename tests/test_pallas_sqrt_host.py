"""CPU: the square root in the pallas base field (csrc/fq29_sqrt.h) and the per-point body of the decompression kernel,
compiled for the host from tests/hosttest/hosttest_sqrt.cpp, against oracle/pallas.py::fq_sqrt.

p - 1 = 2^32 t.  The discrete log in the 2^32-subgroup is what the fixed-trip-count form replaces, so the inputs are
chosen by the order of a^t: for every i in 0 .. 32 at least four a = c^(2^(32 - i)) with c a seeded non-square (a^t has
order exactly 2^i; i = 32 is the non-square itself), plus a = 0, 1, p - 1 and seeded draws."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pallas_decompress_util as U  # noqa: E402

PA, P = U.PA, U.P
ROOT = U.ROOT


@pytest.fixture(scope="module")
def HS(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hosttest_sqrt") / "libhosttest_sqrt.so")
    src = os.path.join(ROOT, "tests", "hosttest", "hosttest_sqrt.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DSNARKV_CURVE_PALLAS", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hs_curve.restype = ctypes.c_char_p
    lib.hs_fq_sqrt.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.hs_g1_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
    lib.hs_g1_decompress.restype = None
    assert lib.hs_curve() == b"pallas"
    return lib


def _sqrt(HS, a):
    out = ctypes.create_string_buffer(32)
    ok = HS.hs_fq_sqrt(a.to_bytes(32, "little"), out)
    return ok, int.from_bytes(out.raw, "little")


def _non_squares(seed, n):
    rnd, out = random.Random(seed), []
    while len(out) < n:
        c = rnd.randrange(1, P)
        if pow(c, (P - 1) // 2, P) == P - 1:
            out.append(c)
    return out


def test_sqrt_for_every_order_of_the_subgroup_part(HS):
    cs = _non_squares(2024, 4)
    seen = {}
    for i in range(33):
        for c in cs:
            a = pow(c, 1 << (32 - i), P)
            assert U.order_exponent(a) == i
            seen[i] = seen.get(i, 0) + 1
            ok, r = _sqrt(HS, a)
            want = PA.fq_sqrt(a)
            if i == 32:
                assert want is None and ok == 0, (i, hex(a))
            else:
                assert ok == 1 and r < P and r * r % P == a, (i, hex(a))
                assert r in (want, P - want)
    assert sorted(seen) == list(range(33)) and min(seen.values()) >= 4


def test_sqrt_of_zero_one_minus_one_and_seeded_draws(HS):
    assert _sqrt(HS, 0) == (1, 0)
    ok, r = _sqrt(HS, 1)
    assert ok == 1 and r in (1, P - 1)
    ok, r = _sqrt(HS, P - 1)  # -1 = g^(2^31): a square, of the highest order a square can have
    assert ok == 1 and r * r % P == P - 1
    assert _sqrt(HS, 5)[0] == 0  # the non-residue the constants are built from
    rnd = random.Random(7)
    squares = 0
    for _ in range(400):
        a = rnd.randrange(P)
        ok, r = _sqrt(HS, a)
        want = PA.fq_sqrt(a)
        assert ok == (want is not None)
        if ok:
            squares += 1
            assert r < P and r * r % P == a
    assert 150 < squares < 250


@pytest.mark.parametrize("mont", [0, 1])
def test_decompress_body_against_the_oracle(HS, mont):
    """The lines k_g1_decompress runs per lane (`g1_decompress_words`): both parities of every seeded x, the identity,
    x = 0 with the parity bit, x >= p, the generator; canonical output and halo2curves' in-memory form.  (The orders of
    the subgroup part are the subject of the first test; tests/test_gpu_pallas_decompress.py asserts their coverage on
    2^15 draws.)"""
    pairs = U.seeded_pairs(11, 150)
    encs = []
    for x, par in pairs:
        encs += [U.encode(x, par), U.encode(x, par ^ 1)]
    encs += [bytes(32), U.encode(0, 1), U.encode(P, 0), U.encode(P + 1, 1), U.encode((1 << 255) - 1, 0), U.encode(P - 1, 0),
             U.encode(P - 1, 1)]
    n = len(encs)
    out, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    HS.hs_g1_decompress(b"".join(encs), n, mont, out, ok)
    good = 0
    for i, e in enumerate(encs):
        want, wok = U.expected(e, bool(mont))
        assert ok.raw[i] == wok, i
        assert out.raw[64 * i:64 * i + 64] == want, i
        good += wok
        if wok and e != bytes(32) and not mont:
            assert out.raw[64 * i + 32] & 1 == e[31] >> 7  # the root emitted has the requested parity
    assert 100 < good < 220
    # x = P - 1 = -1: the generator (-1, 2) and its negative
    g = U.expected(U.encode(P - 1, 0))[0]
    assert int.from_bytes(g[32:], "little") == 2
