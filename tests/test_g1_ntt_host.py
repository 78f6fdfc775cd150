"""CPU: the pass body of the transform over group elements (csrc/g1_ntt.h, the SNARKV_HD source k_g1_ntt_mul and
k_g1_ntt_combine compile) on the host, lane by lane and pass by pass (tests/hosttest/hosttest_g1_ntt.cpp), against the
reference of tests/g1_ntt_util.py (a bit-reversal radix-2 transform on the oracle's point arithmetic, itself held against the
sums of the header by tests/test_g1_ntt_model.py): k = 1, 2, 3 in
both directions on random points and on the inputs that make a butterfly's additions exceptional; the index map of every pass
up to k = 6; the twiddles and n^-1 against Python integers."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import g1_ntt_util as GU  # noqa: E402
import ntt_util as NU  # noqa: E402

CURVES = sorted(GU.CURVES)
_LIBS = {}


def _lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        lib = ctypes.CDLL(mod.build_hosttest("g1_ntt", curve))
        lib.hg_curve.restype = ctypes.c_char_p
        assert lib.hg_curve() == curve.encode()
        lib.hg_max_k.restype = ctypes.c_uint32
        u32, vp = ctypes.c_uint32, ctypes.c_void_p
        for name, args in (("hg_bfly", [u32, u32, u32, vp]), ("hg_twiddle", [u32, u32, u32, vp]), ("hg_n_inverse", [u32, vp]),
                           ("hg_pass", [vp, vp, u32, u32, u32]), ("hg_scale", [vp, vp, u32, vp]), ("hg_transform", [vp, u32, u32])):
            getattr(lib, name).restype, getattr(lib, name).argtypes = None, args
        _LIBS[curve] = lib
    return _LIBS[curve]


def _transform(curve, pts, direction):
    k = len(pts).bit_length() - 1
    io = np.frombuffer(GU.pack(curve, pts), dtype=np.uint32).copy()
    _lib(curve).hg_transform(io.ctypes.data, k, direction)
    return GU.unpack(curve, io.tobytes())


def _scalar(fn, *args):
    out = np.zeros(8, dtype=np.uint32)
    fn(*args, out.ctypes.data)
    return int.from_bytes(out.tobytes(), "little")


@pytest.mark.parametrize("curve", CURVES)
def test_every_pass_reads_and_writes_every_element_once(curve):
    lib = _lib(curve)
    out = np.zeros(5, dtype=np.uint32)
    for k in range(1, 7):
        n = 1 << k
        for s in range(k):
            read, written = [], []
            for j in range(n // 2):
                lib.hg_bfly(k, s, j, out.ctypes.data)
                a, b, lo, hi, e = out.tolist()
                assert (a, b) == (j, j + n // 2) and hi == lo + (1 << s) and e < max(n // 2, 1)
                assert e == (j % (1 << s)) << (k - 1 - s)
                read += [a, b]
                written += [lo, hi]
            assert sorted(read) == sorted(written) == list(range(n)), (k, s)


@pytest.mark.parametrize("curve", CURVES)
def test_twiddles_and_the_inverse_of_n(curve):
    lib, r = _lib(curve), GU.CURVES[curve].R
    assert lib.hg_max_k() >= 20
    for k in (1, 2, 3, 10, 20, lib.hg_max_k()):
        w = NU.omega(curve, k)
        for direction in (GU.FORWARD, GU.INVERSE):
            base = w if direction == GU.FORWARD else pow(w, -1, r)
            for j in sorted({0, 1, 2, (1 << k) // 2 - 1}):
                assert _scalar(lib.hg_twiddle, k, direction, j) == pow(base, j, r), (k, direction, j)
        assert _scalar(lib.hg_n_inverse, k) == pow(1 << k, -1, r)
    assert _scalar(lib.hg_n_inverse, 0) == 1


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_random_points_both_directions(curve, k):
    pts = GU.random_points(curve, 1 << k, "host-%d" % k)
    fwd = _transform(curve, pts, GU.FORWARD)
    assert fwd == GU.reference(curve, pts, GU.FORWARD)
    assert _transform(curve, pts, GU.INVERSE) == GU.reference(curve, pts, GU.INVERSE)
    assert _transform(curve, fwd, GU.INVERSE) == pts


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_exceptional_inputs_both_directions(curve, k):
    for name, pts in GU.special_inputs(curve, 1 << k).items():
        for direction in (GU.FORWARD, GU.INVERSE):
            assert _transform(curve, pts, direction) == GU.reference(curve, pts, direction), (name, direction)


@pytest.mark.parametrize("curve", CURVES)
def test_scale_by_the_scalars_at_the_edges_of_the_split(curve):
    """the pass that multiplies by n^-1, on scalars whose GLV halves are zero, one, or negative: 0, 1, r - 1, lambda-like
    large values"""
    O, lib = GU.CURVES[curve], _lib(curve)
    pts = GU.random_points(curve, 3, "scale") + [None]
    io = np.frombuffer(GU.pack(curve, pts), dtype=np.uint32).copy()
    for e in (0, 1, 2, O.R - 1, O.R - 2, (O.R + 1) // 2, pow(3, -1, O.R), 1 << 127, (1 << 128) - 1):
        ew = np.frombuffer(int(e).to_bytes(32, "little"), dtype=np.uint32).copy()
        out = np.zeros_like(io)
        lib.hg_scale(io.ctypes.data, out.ctypes.data, len(pts), ew.ctypes.data)
        assert GU.unpack(curve, out.tobytes()) == [O.g1_mul(p, e) for p in pts], e
