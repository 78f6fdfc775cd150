"""CPU: the blind term of a blinded commitment (csrc/msm_blind.h, the SNARKV_HD source k_shared_blind compiles) on the host,
lane by lane and level by level (tests/hosttest/hosttest_blind.cpp), against Python integers over the oracles: the digits,
every lane point d_w * 2^(8 w) S, the folded partial blind * S, and the limb bounds of the set S of csrc/g1_29.h at every
lane and level."""
import ctypes
import importlib.util
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

CURVES = {"bn254": BN, "pallas": PA}
W = 32


def _lib(curve):
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build_hosttest("blind", curve))
    lib.hb_curve.restype = ctypes.c_char_p
    assert lib.hb_curve() == curve.encode()
    lib.hb_blind_term.restype = ctypes.c_int
    lib.hb_blind_term.argtypes = [ctypes.c_void_p] * 5
    return lib


def _words(b):
    return np.frombuffer(b, dtype=np.uint32).copy()


def _point(O, words):
    b = words.tobytes()
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
    return None if x == 0 and y == 0 else (x, y)


def _run(O, lib, rows, blind):
    """rows: 32 points -> (digits, lane points, partial)"""
    rw = _words(b"".join(O.g1_to_bytes(p) for p in rows))
    bw = _words(blind.to_bytes(32, "little"))
    digits, lanes, part = np.zeros(W, dtype=np.int32), np.zeros(16 * W, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    rc = lib.hb_blind_term(rw.ctypes.data, bw.ctypes.data, digits.ctypes.data, lanes.ctypes.data, part.ctypes.data)
    assert rc == 0, "carry out of window 31 (1) or a point outside the set S (2): %d" % rc
    return digits.tolist(), [_point(O, lanes[16 * w:16 * w + 16]) for w in range(W)], _point(O, part)


def _recode(s):
    out, carry = [], 0
    for w in range(W):
        raw = ((s >> (8 * w)) & 0xFF) + carry
        carry = 1 if raw > 128 else 0
        out.append(raw - 256 * carry)
    assert carry == 0
    return out


def _table(O, s):
    rows = [s]
    for _ in range(W - 1):
        p = rows[-1]
        for _ in range(8):
            p = O.g1_double(p)
        rows.append(p)
    return rows


def _blinds(O):
    rnd = random.Random("blind-" + str(O.R % 1000))
    return [0, 1, O.R - 1,
            int.from_bytes(b"\x80" * 32, "little"),  # the recoding's carry chain; above r: counts mod r
            (O.R >> 248) << 248,                     # only the top digit set (below r)
            0x7F, 0x80, 0x81, 0xFF, (O.R - 1) // 2, O.R, O.R + 1, (1 << 256) - 1] + [rnd.randrange(O.R) for _ in range(24)]


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_blind_term_lane_by_lane_against_the_oracle(curve):
    O, lib = CURVES[curve], _lib(curve)
    s = O.g1_mul(O.G1_GEN, 0xB11D5EED)
    rows = _table(O, s)
    assert rows[3] == O.g1_mul(s, 1 << 24)
    for blind in _blinds(O):
        digits, lanes, part = _run(O, lib, rows, blind)
        want = _recode(blind % O.R)
        assert digits == want, hex(blind)
        assert min(digits) >= -127 and max(digits) <= 128
        for w in range(W):
            assert lanes[w] == O.g1_mul(rows[w], want[w] % O.R), (hex(blind), w)
        assert part == O.g1_mul(s, blind % O.R), hex(blind)
    # every magnitude a digit can take, with both signs, on one row
    for d in list(range(1, 129)) + [256 - m for m in range(1, 128)]:
        digits, lanes, part = _run(O, lib, rows, d)
        sd = d if d <= 128 else d - 256
        assert digits[0] == sd and lanes[0] == O.g1_mul(s, sd % O.R)
        assert part == O.g1_mul(s, d)


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_equal_opposite_and_identity_points_meet_in_the_fold(curve):
    """rows that are not a doubling chain: S and -S, S and S, and identity rows meet in the tree, where the careful addition
    has to cancel, double and skip"""
    O, lib = CURVES[curve], _lib(curve)
    s = O.g1_mul(O.G1_GEN, 77)
    same = [s] * W
    # digits +1 at every window: 32 equal points, doubled level by level -> 32 S
    assert _run(O, lib, same, int.from_bytes(b"\x01" * 32, "little"))[2] == O.g1_mul(s, 32)
    # 0xFF -> digits (-1, +1): -S and S meet at the last level -> the identity
    digits, lanes, part = _run(O, lib, same, 0xFF)
    assert digits[:2] == [-1, 1] and lanes[0] == O.g1_neg(s) and lanes[1] == s and part is None
    # windows 0 and 16 are partners at the FIRST level: S + (-S) there, and the rest still sums
    rows = list(same)
    rows[16] = O.g1_neg(s)
    blind = 1 | (1 << 128) | (5 << 8)
    assert _run(O, lib, rows, blind)[2] == O.g1_mul(s, 5)
    # S + S at the first level (a doubling), plus an identity row whose digit is not zero
    rows = list(same)
    rows[2] = None
    blind = 3 | (3 << 128) | (9 << 16)
    digits, lanes, part = _run(O, lib, rows, blind)
    assert lanes[2] is None and part == O.g1_mul(s, 6)
    # all rows identity
    assert _run(O, lib, [None] * W, O.R - 1)[2] is None
