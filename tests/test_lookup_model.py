"""CPU: the lookup argument's shared logic (snark-verifier_amd/csrc/lookup.h, the source the device compiles), run on the host
through tests/hosttest/hosttest_lookup.cpp for both curves with tiles and scan blocks of 2, 3, 4 and 8 elements, so that every
border is hit, against Python integers (tests/lookup_util.py): the comparison on keys that differ in one word only; the
merge-path partition at every diagonal of short runs with many ties; the whole tiled sort at every length 1 to 40, out of place
and in place; and the permute rule against the sequential model on every (A, S) pair with u <= 6 over {0, 1, 2}, missing values
included.  Every comparison is on canonical words, nothing is filtered."""
import ctypes
import importlib.util
import itertools
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lookup_util as LU  # noqa: E402

CURVES = ["bn254", "pallas"]
TILES = [2, 3, 4, 8]
_LIBS = {}
_u32p = ctypes.POINTER(ctypes.c_uint32)


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("lookup", curve))
        lib.hl_curve.restype = ctypes.c_char_p
        for fn in (lib.hl_less, lib.hl_equal, lib.hl_permute):
            fn.restype = ctypes.c_int
        for fn in (lib.hl_merge_path, lib.hl_passes):
            fn.restype = ctypes.c_uint32
        lib.hl_canon.restype = lib.hl_sort.restype = None
        assert lib.hl_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


def _words(vals):
    raw = LU.pack(vals) or b"\x00" * 32
    return (ctypes.c_uint32 * (len(raw) // 4)).from_buffer_copy(raw)


def _filled(n_elems):
    return (ctypes.c_uint32 * (8 * n_elems + 8))(*([0xAAAAAAAA] * (8 * n_elems + 8)))


def _vals(buf, n):
    raw = bytes(buf)
    assert raw[32 * n:] == b"\xaa" * 32  # the guard behind it
    return LU.unpack(raw[:32 * n])


@pytest.mark.parametrize("curve", CURVES)
def test_comparison_against_integers(curve):
    lib, r = host_lib(curve), LU.FIELD[curve]
    rnd = random.Random("lookup-model-compare-" + curve)
    pairs = []
    for word in (0, 3, 7):  # keys that differ only in the lowest word, in one middle word, only in the highest
        for _ in range(50):
            base = rnd.randrange(1 << 256) & ~(0xFFFFFFFF << (32 * word))
            x, y = rnd.sample(range(1 << 32), 2)
            pairs += [(base | x << (32 * word), base | y << (32 * word))]
        base = rnd.randrange(1 << 256) & ~(0xFFFFFFFF << (32 * word))
        pairs += [(base, base | 1 << (32 * word)), (base | 0xFFFFFFFF << (32 * word), base | 0xFFFFFFFE << (32 * word))]
    pairs += [(rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(200)]
    pairs += [(0, 0), (0, 1), ((1 << 256) - 1, (1 << 256) - 1), ((1 << 256) - 1, 0), (1 << 255, (1 << 255) - 1), (1 << 32, (1 << 32) - 1)]
    for a, b in pairs:
        for x, y in ((a, b), (b, a), (a, a)):  # both ways round, and equal
            assert lib.hl_less(_words([x]), _words([y])) == int(x < y), (hex(x), hex(y))
            assert lib.hl_equal(_words([x]), _words([y])) == int(x == y), (hex(x), hex(y))
    for v in (0, 1, r - 1, r, r + 1, 2 * r, (1 << 256) - 1, rnd.randrange(1 << 256)):  # an input >= r is taken mod r
        out = _filled(1)
        lib.hl_canon(_words([v]), out)
        assert _vals(out, 1) == [v % r], hex(v)


@pytest.mark.parametrize("curve", CURVES)
def test_merge_path_at_every_diagonal(curve):
    lib = host_lib(curve)
    rnd = random.Random("lookup-model-path-" + curve)
    shapes = [(0, 5), (5, 0), (1, 1), (3, 8), (8, 3), (7, 7), (9, 12)]
    for na, nb in shapes:
        for spread in (1, 2, 4, 1 << 200):  # spread 1: all equal; small spreads: many ties
            a = sorted(rnd.randrange(spread) for _ in range(na))
            b = sorted(rnd.randrange(spread) for _ in range(nb))
            merged = sorted(a + b)
            wa, wb = _words(a), _words(b)
            last = 0
            for diag in range(na + nb + 1):
                i = lib.hl_merge_path(wa, na, wb, nb, diag)
                j = diag - i
                assert 0 <= i <= na and 0 <= j <= nb and i >= last, (na, nb, spread, diag)
                assert sorted(a[:i] + b[:j]) == merged[:diag]  # the two counts add up to the first diag of the merge
                # "a first": no taken element of b equals an element of a that is left behind
                assert not (j and i < na and a[i] <= b[j - 1]), (na, nb, spread, diag)
                last = i


@pytest.mark.parametrize("curve", CURVES)
def test_tiled_sort_at_every_length(curve):
    lib, r = host_lib(curve), LU.FIELD[curve]
    for tile in TILES:
        for lane_e in (1, 2) if tile > 2 else (1,):
            for n in range(1, 41):
                rnd = random.Random("lookup-model-sort-%s-%d-%d" % (curve, tile, n))
                for name, vals in (("uniform", [rnd.randrange(1 << 256) for _ in range(n)]),
                                   ("ties", [rnd.randrange(3) for _ in range(n)]),
                                   ("equal", [r + 5] * n),
                                   ("reversed", list(range(n, 0, -1)))):
                    want = LU.sort_model(vals, r)
                    src, work, out = _words(vals), _filled(n), _filled(n)
                    lib.hl_sort(src, n, tile, lane_e, work, out)
                    assert _vals(out, n) == want, (tile, lane_e, n, name)
                    _vals(work, n)  # its guard
                    inplace = _filled(n)
                    ctypes.memmove(inplace, src, 32 * n)
                    lib.hl_sort(inplace, n, tile, lane_e, work, inplace)
                    assert _vals(inplace, n) == want, (tile, lane_e, n, name, "in place")
    assert [lib.hl_passes(n, 4) for n in (1, 4, 5, 8, 9, 16, 17)] == [0, 0, 1, 1, 2, 2, 3]


def _run_permute(lib, A, S, u, tile, block):
    work, pi, pt, st = _filled(2 * u), _filled(u), _filled(u), (ctypes.c_uint32 * 5)(*([0xAAAAAAAA] * 5))
    assert lib.hl_permute(_words(A), _words(S), u, tile, 1, block, work, pi, pt, st) == 0
    _vals(work, 2 * u)
    assert st[4] == 0xAAAAAAAA
    return _vals(pi, u), _vals(pt, u), list(st[:4])


@pytest.mark.parametrize("curve", CURVES)
def test_permute_rule_exhaustively(curve):
    lib, r = host_lib(curve), LU.FIELD[curve]
    geometry = [(2, 2), (3, 3), (4, 4), (8, 8), (2, 3), (4, 2), (3, 8), (8, 4)]  # (sort tile, scan block)
    for u in range(1, 7):
        rows = list(itertools.product(range(3), repeat=u))
        words = {t: _words(t) for t in rows}
        model = {}  # the model sorts A and counts S: one evaluation per pair of multisets
        work, pi, pt, st = _filled(2 * u), _filled(u), _filled(u), (ctypes.c_uint32 * 5)()
        at = 0
        for A in rows:
            for S in rows:
                key = (tuple(sorted(A)), tuple(sorted(S)))
                if key not in model:
                    model[key] = LU.permute_model(list(A), list(S), u, r)
                    assert LU.constraints_hold(A, S, model[key][0], model[key][1], u, r) == (model[key][2][0] == 0)
                want = model[key]
                # every geometry for u < 5, one per pair in turn above (4 of the 8 at u = 5)
                for g in range(len(geometry) if u < 5 else (4 if u == 5 else 1)):
                    tile, block = geometry[(at + g) % len(geometry)]
                    at += 1
                    for buf in (work, pi, pt, st):
                        ctypes.memset(buf, 0xAA, ctypes.sizeof(buf))
                    assert lib.hl_permute(words[A], words[S], u, tile, 1, block, work, pi, pt, st) == 0
                    got = (_vals(pi, u), _vals(pt, u), list(st[:4]))
                    assert got == want and st[4] == 0xAAAAAAAA, (A, S, tile, block)
                    _vals(work, 2 * u)


@pytest.mark.parametrize("curve", CURVES)
def test_permute_larger_cases_with_tiny_blocks(curve):
    """the issue's cases at sizes where the scans have three levels of blocks of 2 or 3"""
    lib, r = host_lib(curve), LU.FIELD[curve]
    for u, tile, block in ((23, 4, 2), (40, 8, 3), (70, 8, 4), (300, 8, 8)):
        for name, (A, S, missing) in LU.permute_cases(u, r, tile, block, "model-" + curve).items():
            want = LU.permute_model(A, S, u, r)
            assert want[2][0] == missing, name
            assert _run_permute(lib, A, S, u, tile, block) == want, (u, name)
            assert LU.constraints_hold(A, S, want[0], want[1], u, r) == (missing == 0), (u, name)
