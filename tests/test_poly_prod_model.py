"""CPU: the blocked product scans behind `snarkv_poly_batch_invert_dev` and `snarkv_poly_grand_product_dev`
(snark-verifier_amd/csrc/poly_prod.h, the source the device compiles), run on the host through
tests/hosttest/hosttest_poly_prod.cpp for both curves against Python integers: blocks of 2, 3 and 4 elements (the last as two
lanes of two, the shape of the device's level 0) at lengths up to 65, which is seven levels with blocks of 2.

Inputs: random values, all r - 1, all 1, zeros planted at the ends, on both sides of a block boundary and over one whole block,
the all-zero input, and one element spelt as the words of r, which counts as zero.  Nothing is filtered: every output is
compared, the zeros included."""
import ctypes
import importlib.util
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
BLOCKS = [2, 3, 4]
LENGTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65]
_LIBS = {}
_u32p = ctypes.POINTER(ctypes.c_uint32)


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("poly_prod", curve))
        lib.hpp_curve.restype = ctypes.c_char_p
        lib.hpp_grand_product.restype = ctypes.c_uint32
        lib.hpp_batch_invert.restype = ctypes.c_uint32
        lib.hpp_affine_step.restype = None
        assert lib.hpp_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


def _words(vals):
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return (ctypes.c_uint32 * (8 * len(vals))).from_buffer_copy(raw)


def _ints(arr):
    raw = bytes(arr)
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def levels(n, block):
    """the block of 4 is two lanes of two elements, so its totals are scanned two to a block (hosttest_poly_prod.cpp)"""
    count = 1
    while -(-n // block) > 1:
        n, block = -(-n // block), 2 if block == 4 else block
        count += 1
    return count


def batch_invert(curve, vals, block):
    lib, n = host_lib(curve), len(vals)
    out, inv = (ctypes.c_uint32 * (8 * n))(), ctypes.c_uint32(0)
    got = lib.hpp_batch_invert(_words(vals), n, block, out, ctypes.byref(inv))
    assert got == levels(n, block), (n, block, got)
    assert inv.value == 1, "one field inversion per call"
    return _ints(out)


def grand_product(curve, vals, block, start=None):
    lib, n = host_lib(curve), len(vals)
    out, total = (ctypes.c_uint32 * (8 * n))(), (ctypes.c_uint32 * 8)()
    got = lib.hpp_grand_product(_words(vals), n, _words([start]) if start is not None else None, block, out, total)
    assert got == levels(n, block), (n, block, got)
    return _ints(out), _ints(total)[0]


def inputs(curve, n, block):
    """name -> values; r itself stands for the 32 bytes that spell r"""
    r = FIELD[curve]
    rnd = random.Random("poly-prod-model-%s-%d-%d" % (curve, n, block))
    base = [rnd.randrange(1, r) for _ in range(n)]
    cases = {"random": base, "all r-1": [r - 1] * n, "all one": [1] * n, "all zero": [0] * n}

    def planted(where):
        v = list(base)
        for i in where:
            v[i] = 0
        return v

    cases["zero at 0"] = planted([0])
    cases["zero at n-1"] = planted([n - 1])
    if n > block:
        cases["zeros around a block boundary"] = planted([block - 1, block])
        cases["a whole block of zeros"] = planted(range(block, min(2 * block, n)))
    cases["the words of r"] = base[:n // 2] + [r] + base[n // 2 + 1:]
    return cases


def test_lengths_reach_seven_levels():
    assert max(levels(n, 2) for n in LENGTHS) == 7 and levels(65, 2) == 7 and levels(64, 2) == 6


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_batch_inverse(curve, block, n):
    r = FIELD[curve]
    for name, vals in inputs(curve, n, block).items():
        got = batch_invert(curve, vals, block)
        for i, (x, y) in enumerate(zip(vals, got)):
            assert 0 <= y < r, (name, i)
            if x % r == 0:
                assert y == 0, (name, i)
            else:
                assert x * y % r == 1, (name, i)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_grand_product(curve, block, n):
    r = FIELD[curve]
    rnd = random.Random("poly-prod-model-start-%s" % curve)
    for name, vals in inputs(curve, n, block).items():
        for start in (None, 0, 1, r - 1, rnd.randrange(r)):
            want, acc = [], 1 if start is None else start
            for x in vals:
                want.append(acc)
                acc = acc * x % r
            out, total = grand_product(curve, vals, block, start)
            assert out == want, (name, start)
            assert total == acc, (name, start)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_affine_term_at_its_largest_sums(curve):
    """a + beta b + gamma with every part r - 1, 0, or random: the sum the stated bound (-3r/2, 9r/2) is for"""
    r, lib = FIELD[curve], host_lib(curve)
    rnd = random.Random("poly-prod-model-affine-%s" % curve)
    edge = [0, 1, r - 1]
    cases = [(acc, a, b, be, ga) for acc in (1, r - 1) for a in edge for b in edge for be in edge for ga in edge]
    cases += [tuple(rnd.randrange(r) for _ in range(5)) for _ in range(64)]
    cases.append((r - 1, r - 1, r, r - 1, r - 1))  # a column element spelt as r is zero
    out = (ctypes.c_uint32 * 8)()
    for acc, a, b, be, ga in cases:
        for has_b in (1, 0):
            lib.hpp_affine_step(_words([acc]), _words([a]), _words([b]), _words([be]), _words([ga]), has_b, out)
            assert _ints(out)[0] == acc * (a + (be * b if has_b else 0) + ga) % r, (acc, a, b, be, ga, has_b)
