"""CPU: the argument checks that the entry points of the resident-polynomial units share (snark-verifier_amd/csrc/poly_args.hpp),
run on the host through tests/hosttest/hosttest_args.cpp for both curves against Python integers, which cannot wrap: the
overlap of two byte ranges (empty, adjacent, nested, identical, and within 64 bytes of 2^64, where a test written on
`address + length` wraps), the saturating byte count, the canonical test of a scalar around r, and the index and overlap
checks of a call on columns."""
import ctypes
import importlib.util
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
OK, EMPTY, LENGTH, ARG = 0, -1, -2, -5  # include/snarkv_amd.h
NONE = 0xFFFFFFFF  # SNARKV_POLY_NONE
_u64, _u64p, _u32p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
_LIBS = {}


def host_lib(curve):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("args", curve))
        lib.har_curve.restype = lib.har_last_error.restype = ctypes.c_char_p
        lib.har_overlap.argtypes = [_u64] * 4
        lib.har_partial_overlap.argtypes = [_u64] * 3
        lib.har_aligned16.argtypes = [_u64]
        lib.har_bytes_of.restype, lib.har_bytes_of.argtypes = _u64, [_u64]
        lib.har_check_len.argtypes = [_u64, _u64]
        lib.har_all_below_r.argtypes = [ctypes.c_char_p, _u64]
        lib.har_check_columns.argtypes = [_u64, _u64, _u64, _u32p, _u64, ctypes.c_char_p, _u64, _u64p, _u64p, _u64]
        assert lib.har_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


def overlap(a, an, b, bn):
    """two byte ranges as sets of integers: no modulus anywhere"""
    return an > 0 and bn > 0 and a < b + bn and b < a + an


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_the_edge_cases_as_the_host_runs_them_on_constants(curve):
    assert host_lib(curve).har_selftest() == 0


def test_overlap_is_the_overlap_of_integer_ranges_up_to_the_top_of_the_address_space():
    lib = host_lib("bn254")
    top = 1 << 64
    bases = [0x1000, 0x1001, 0x1020, 0x103F, 0x1040, top - 64, top - 33, top - 32, top - 31, top - 1]
    lengths = [0, 1, 31, 32, 33, 64]
    seen = set()
    for a, an, b, bn in itertools.product(bases, lengths, bases, lengths):
        if a + an > top or b + bn > top:  # a buffer does not run past the address space
            continue
        want = overlap(a, an, b, bn)
        assert bool(lib.har_overlap(a, an, b, bn)) == want, (hex(a), an, hex(b), bn)
        seen.add(want)
        if an == bn:
            assert bool(lib.har_partial_overlap(a, b, an)) == (a != b and want), (hex(a), hex(b), an)
    assert seen == {False, True}
    # where `x < y + bn && y < x + an` on 64-bit words goes wrong: y + bn wraps to 0, and the two ranges do share bytes
    a, an, b, bn = top - 64, 64, top - 32, 32
    assert overlap(a, an, b, bn) and not (a < (b + bn) % top and b < (a + an) % top)
    assert lib.har_overlap(a, an, b, bn) and lib.har_overlap(b, bn, a, an)
    for p, want in ((0, False), (16, True), (0x1008, False), (0x100F, False), (0x1010, True), (top - 16, True), (top - 1, False)):
        assert bool(lib.har_aligned16(p)) == want, hex(p)


def test_bytes_of_saturates_and_check_len_orders_its_codes():
    lib = host_lib("bn254")
    for n in (0, 1, 2, 1 << 30, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, 1 << 58, 1 << 59, 1 << 63, (1 << 64) - 1):
        want = 32 * n if n <= 1 << 40 else 1 << 45
        assert lib.har_bytes_of(n) == want, n
    for n, cap, want in ((0, 8, EMPTY), (0, 0, EMPTY), (1, 8, OK), (8, 8, OK), (9, 8, LENGTH), (1 << 30, 1 << 30, OK),
                         ((1 << 30) + 1, 1 << 30, LENGTH), ((1 << 64) - 1, 1 << 30, LENGTH)):
        assert lib.har_check_len(n, cap) == want, (n, cap)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_below_r_is_the_integer_comparison(curve):
    lib, r = host_lib(curve), FIELD[curve]
    fe = lambda v: v.to_bytes(32, "little")  # noqa: E731
    values = [0, 1, r - 1, r, r + 1, (1 << 256) - 1, r - (1 << 224), r + (1 << 224), r ^ 1 << 255, r & ((1 << 32) - 1)]
    for v in values:
        assert bool(lib.har_below_r(fe(v))) == (v < r), hex(v)
        assert bool(lib.har_is_zero32(fe(v))) == (v == 0), hex(v)
    assert lib.har_all_below_r(b"", 0) and lib.har_all_below_r(fe(0) + fe(r - 1), 2)
    for bad in range(3):
        vals = [0, 1, r - 1]
        vals[bad] = r
        assert not lib.har_all_below_r(b"".join(fe(v) for v in vals), 3), bad
        assert lib.har_all_below_r(b"".join(fe(v) for v in vals), bad)  # the scalars before it are canonical


def check_columns_model(polys, n, n_polys, idx, none_ok, outs):
    """-> (code, the word of the refusal): the arrays in turn, in each the indices in turn, an index before its overlaps"""
    if n_polys == 0:
        return OK, None
    col = 32 * n
    for arr, lax in zip(idx, none_ok):
        for i in arr:
            if i == NONE and lax:
                continue
            if i >= n_polys:
                return ARG, "index %d" % i
            if any(overlap(o, ob, polys + col * i, col) for o, ob in outs):
                return ARG, "column %d" % i
    return OK, None


def test_check_columns_refuses_what_the_model_refuses_and_names_it():
    lib = host_lib("bn254")
    polys, n, n_polys, far = 0x10000, 4, 3, 0x80000
    col = 32 * n
    last32 = polys + 2 * col - 32  # the last 32 bytes of column 1

    def run(idx, none_ok, outs, columns=n_polys):
        count = len(idx[0])
        flat = [i for arr in idx for i in arr]
        o = (_u64 * len(outs))(*[a for a, _ in outs])
        ob = (_u64 * len(outs))(*[b for _, b in outs])
        lib.har_clear_error()
        rc = lib.har_check_columns(polys, n, columns, (ctypes.c_uint32 * max(len(flat), 1))(*flat), len(idx), bytes(none_ok),
                                   count, o, ob, len(outs))
        want, word = check_columns_model(polys, n, columns, idx, none_ok, outs)
        assert rc == want, (idx, none_ok, outs, columns)
        text = lib.har_last_error().decode()
        assert (word in text and ("index" in text or "overlap" in text)) if word else text == "", text
        return rc

    out = [(far, col)]
    assert run([[0, 1], [2, 0]], [0, 0], out) == OK
    assert run([[0, 1], [3, 0]], [0, 0], out) == ARG  # an index equal to n_polys
    assert run([[0, 1], [0, NONE]], [0, 1], out) == OK and run([[0, 1], [0, NONE]], [0, 0], out) == ARG
    assert run([[NONE, 1], [0, 0]], [0, 1], out) == ARG  # allowed in the second array only
    assert run([[0, 1], [3, NONE]], [0, 0], out, columns=0) == OK  # nothing to index
    assert run([[0, 1], [0, 1]], [0, 0], [(last32, 32)]) == ARG and run([[0, 2], [2, 0]], [0, 0], [(last32, 32)]) == OK
    assert run([[0, 1], [0, 1]], [0, 0], [(last32 + 32, 32)]) == OK  # the first byte after the column
    assert run([[0, 1], [0, 1]], [0, 0], [(polys + col - 1, 1)]) == ARG and run([[1], [1]], [0, 0], [(polys + col - 1, 1)]) == OK
    # the refusal that comes first: array by array, and in one entry the index before the overlap
    assert run([[1, 0], [3, 0]], [0, 0], [(last32, 32)]) == ARG and "column 1" in lib.har_last_error().decode()
    assert run([[3, 1], [0, 0]], [0, 0], [(last32, 32)]) == ARG and "index 3" in lib.har_last_error().decode()
    # several outputs, one of them empty (a total that is not asked for), and no entries at all
    assert run([[0], [1], [2]], [0, 0, 0], [(far, 2 * col), (far + 2 * col, col), (polys, 0)]) == OK
    assert run([[0], [1], [2]], [0, 0, 0], [(far, 2 * col), (far + 2 * col, col), (polys + 2 * col, 32)]) == ARG
    assert run([[], []], [0, 0], [(polys, col)]) == OK
