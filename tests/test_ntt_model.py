"""CPU: the transform behind `snarkv_ntt_dev` (snark-verifier_amd/csrc/ntt_plan.h and ntt_tile.h, the source the device
compiles), run on the host through tests/hosttest/hosttest_ntt.cpp for both curves against the reference of tests/ntt_util.py:
tiles of 2^1, 2^2 and 2^3 elements at k = 0 .. 10 (up to ten passes), the device's tile of 2^9 on both sides of one pass, every
pass of every plan as a permutation, and the largest multiplier input against the bound ntt_tile.h derives.

The bound.  ntt_tile.h reduces after every sixth level and states 7.5 r for the largest multiplier input (7 x 1.07 r: six
levels of growth on top of a fresh value).  `test_reduction_schedule_keeps_the_bound` recomputes that recurrence from the
schedule the library exports (`hn_reduce_after`, the function the kernel calls) and holds what the model measured against it,
pass depth by pass depth.  Moving the schedule one level later (`level && level % 6 == 0`) was tried once: the recurrence
gives 8.56 r at the reduction and the test fails.  Measured maxima on the worst-value inputs at the device's tile, k = 8, 9,
10: 5.000, 5.000, 4.740 on BN254 and 7.000, 7.000, 6.000 on pallas (a constant input makes the top operand of every level the
same residue, so the sum before the reduction is seven times it)."""
import ctypes
import importlib.util
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ntt_util as U  # noqa: E402

CURVES = sorted(U.CURVES)
DEVICE_T = 9
GROWTH = 1.07  # of a top operand per level, in units of r (ntt_tile.h: a product with a canonical operand is in (-0.07r, 1.07r))
_LIBS = {}


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("ntt", curve))
        lib.hn_curve.restype = ctypes.c_char_p
        lib.hn_bound.restype = ctypes.c_double
        lib.hn_max.restype = ctypes.c_double
        assert lib.hn_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


def _words(vals):
    return np.frombuffer(U.pack(vals), dtype=np.uint32).copy()


def run(lib, vals, direction, shift, tile_bits):
    n, vp = len(vals), ctypes.c_void_p
    k = n.bit_length() - 1
    out = np.zeros(8 * n, dtype=np.uint32)
    sh = None if shift is None else _words([shift]).ctypes.data_as(vp)
    assert lib.hn_ntt(_words(vals).ctypes.data_as(vp), out.ctypes.data_as(vp), k, direction, sh, tile_bits) == 1
    return U.unpack(out.tobytes())


def plan(lib, k, tile_bits):
    t, c = (ctypes.c_uint32 * 32)(), (ctypes.c_uint32 * 32)()
    passes = lib.hn_plan(k, tile_bits, t, c)
    assert passes >= 1
    return list(t[:passes]), list(c[:passes])


@pytest.mark.parametrize("curve", CURVES)
def test_reference_is_the_definition_and_the_constants_are_the_oracles(curve):
    r = U.CURVES[curve].R
    rnd = random.Random("ntt-def-" + curve)
    vals, s = [rnd.randrange(r) for _ in range(8)], rnd.randrange(1, r)
    for direction in (U.FORWARD, U.INVERSE):
        for shift in (None, s):
            assert U.reference(curve, vals, direction, shift) == U.definition(curve, vals, direction, shift)
    assert U.reference(curve, U.reference(curve, vals, U.FORWARD, s), U.INVERSE, pow(s, -1, r)) == vals
    assert host_lib(curve).hn_two_adicity() == U.CURVES[curve].TWO_ADICITY


@pytest.mark.parametrize("tile_bits", [1, 2, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_small_tiles_equal_the_reference(curve, tile_bits):
    r, lib = U.CURVES[curve].R, host_lib(curve)
    rnd = random.Random("ntt-model-%s-%d" % (curve, tile_bits))
    for k in range(0, 11):
        vals, s = [rnd.randrange(r) for _ in range(1 << k)], rnd.randrange(1, r)
        for direction in (U.FORWARD, U.INVERSE):
            for shift in (None, s):
                assert run(lib, vals, direction, shift, tile_bits) == U.reference(curve, vals, direction, shift), (k, direction, shift)


@pytest.mark.parametrize("k", [DEVICE_T - 1, DEVICE_T, DEVICE_T + 1])
@pytest.mark.parametrize("curve", CURVES)
def test_device_tile_equals_the_reference(curve, k):
    r, lib = U.CURVES[curve].R, host_lib(curve)
    rnd = random.Random("ntt-model-dev-%s-%d" % (curve, k))
    vals, s = [rnd.randrange(r) for _ in range(1 << k)], rnd.randrange(1, r)
    for direction in (U.FORWARD, U.INVERSE):
        for shift in (None, s):
            assert run(lib, vals, direction, shift, DEVICE_T) == U.reference(curve, vals, direction, shift), (direction, shift)


@pytest.mark.parametrize("tile_bits", [1, 2, 3, DEVICE_T])
def test_every_pass_is_a_permutation(tile_bits):
    lib = host_lib("bn254")  # index arithmetic only: the same on both curves
    vp = ctypes.c_void_p
    for k in list(range(0, 13)) + ([14, 15, 16] if tile_bits == DEVICE_T else []):
        n = 1 << k
        t, c = plan(lib, k, tile_bits)
        assert sum(t) == k and all(ti + ci <= tile_bits for ti, ci in zip(t, c))
        if k <= tile_bits:
            assert t == [k]  # one pass of one tile
        else:
            assert all(1 <= ti for ti in t) and max(t) - min(t) <= 1  # spread evenly
        everything = np.arange(n, dtype=np.uint32)
        stored_before = None
        for p in range(len(t)):
            arrs = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
            assert lib.hn_pass_indices(k, tile_bits, p, *[a.ctypes.data_as(vp) for a in arrs]) == 1
            load, store, lds_load, lds_store = arrs
            # each index is loaded once and stored once
            assert np.array_equal(np.sort(load), everything) and np.array_equal(np.sort(store), everything), (k, p)
            if stored_before is not None:  # ... and a pass loads what the pass before stored
                assert np.array_equal(np.sort(load), np.sort(stored_before))
            stored_before = store
            slots = 1 << (t[p] + c[p])
            for g in range(n // slots):
                tl = slice(g * slots, (g + 1) * slots)
                # within a tile every LDS place is written once by the loads and read once by the stores
                assert np.array_equal(np.sort(lds_load[tl]), np.arange(slots)) and np.array_equal(np.sort(lds_store[tl]), np.arange(slots))
                if p + 1 < len(t):  # a pass before the last stores where it loaded: it may run in place
                    assert np.array_equal(np.sort(load[tl]), np.sort(store[tl])), (k, p, g)
            if p + 1 < len(t) and c[p]:  # rows are runs of 2^c consecutive elements
                runs = load.reshape(-1, 1 << c[p])
                assert np.all(np.diff(runs.astype(np.int64), axis=1) == 1), (k, p)
            if p + 1 == len(t) and len(t) > 1:  # the last pass loads runs of 2^t and stores runs of 2^c
                assert np.all(np.diff(load.reshape(-1, 1 << t[p]).astype(np.int64), axis=1) == 1), (k, p)
                assert np.all(np.diff(store.reshape(-1, 1 << c[p]).astype(np.int64), axis=1) == 1), (k, p)


def worst_inputs(r, n):
    """all r - 1, all 1, and a single r - 1 at index 0, 1 and n - 1"""
    out = [[r - 1] * n, [1] * n]
    for at in sorted({0, 1 % n, n - 1}):
        v = [0] * n
        v[at] = r - 1
        out.append(v)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_reduction_schedule_keeps_the_bound(curve):
    r, lib = U.CURVES[curve].R, host_lib(curve)
    stated = lib.hn_bound()
    assert stated < 8.0
    # the recurrence of ntt_tile.h's comment over the schedule the kernel uses: a fresh value is below GROWTH r, a level adds
    # GROWTH r, the reduction after a level takes what that level made and leaves a fresh value
    bound_in, largest = GROWTH, 0.0
    per_levels = {}  # levels of a pass -> largest multiplier input in a pass of that many levels
    for level in range(DEVICE_T):
        largest = max(largest, bound_in)  # the bottom operand of the butterfly
        bound_in += GROWTH
        if lib.hn_reduce_after(level):
            largest = max(largest, bound_in)  # the reduction's own input
            bound_in = GROWTH
        per_levels[level + 1] = max(largest, bound_in)  # ... and what the store multiplies
    assert max(per_levels.values()) < stated, per_levels
    assert any(lib.hn_reduce_after(level) for level in range(DEVICE_T))
    # what the model meets on the worst inputs, at the device's tile: below the recurrence's figure for the deepest pass
    s = random.Random("ntt-bound-" + curve).randrange(1, r)
    for k in (DEVICE_T - 1, DEVICE_T, DEVICE_T + 1):
        t, _ = plan(lib, k, DEVICE_T)
        limit = per_levels[max(t)] if max(t) else GROWTH
        for vals in worst_inputs(r, 1 << k):
            for direction, shift in ((U.FORWARD, None), (U.INVERSE, None), (U.FORWARD, s), (U.INVERSE, r - 1)):
                lib.hn_reset_max()
                assert run(lib, vals, direction, shift, DEVICE_T) == U.reference(curve, vals, direction, shift)
                seen = lib.hn_max()
                print("ntt bound %s k=%d dir=%d shift=%s levels=%s: max |input|/r = %.3f (limit %.2f, stated %.2f)" % (
                    curve, k, direction, shift is not None, t, seen, limit, stated))
                assert 0.0 < seen < limit <= stated
