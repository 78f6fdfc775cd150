"""CPU: the shared-key MSM of csrc/msm_shared.hip in exact integers over the oracles -- the window table
T[w][j] = 2^(8 w) G[j], signed 8-bit digits, ONE set of 128 buckets, sum_b b B_b -- against the oracle MSM; and the
recoder itself (csrc/msm_shared.h, the source the device compiles) as a raw op in the style of
tests/hosttest/curve_ops.h (tests/hosttest/hosttest_shared.cpp), in a host library per curve."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

C_BITS, W, BUCKETS = 8, 32, 128
CURVES = {"bn254": BN, "pallas": PA}


def recode(s):
    """the signed digits of msm_shared.h: low to high, a raw byte plus carry above 128 becomes raw - 256 with a carry up"""
    out, carry = [], 0
    for w in range(W):
        raw = ((s >> (C_BITS * w)) & 0xFF) + carry
        carry = 1 if raw > 128 else 0
        out.append(raw - 256 * carry)
    return out, carry


def shared_msm(O, table, scalars):
    """one bucket set for the whole vector, then the running sum from the top bucket down"""
    buckets = [None] * (BUCKETS + 1)
    for j, s in enumerate(scalars):
        digits, carry = recode(s % O.R)
        assert carry == 0
        for w, d in enumerate(digits):
            if d:
                p = table[w][j]
                buckets[abs(d)] = O.g1_add(buckets[abs(d)], p if d > 0 else O.g1_neg(p))
    run = acc = None
    for b in range(BUCKETS, 0, -1):
        run = O.g1_add(run, buckets[b])
        acc = O.g1_add(acc, run)
    return acc


@pytest.mark.parametrize("curve", sorted(CURVES))
@pytest.mark.parametrize("k", [1, 3, 6])
def test_single_bucket_set_over_the_window_table_equals_the_oracle_msm(curve, k):
    O = CURVES[curve]
    rnd = random.Random("model-%s-%d" % (curve, k))
    n = 1 << k
    g = [O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R)) for _ in range(n)]
    if k == 6:
        g[9], g[6], g[11] = g[3], O.g1_neg(g[5]), None  # equal, opposite and identity rows
    table = [g]
    for w in range(1, W):
        row = table[-1]
        for _ in range(C_BITS):
            row = [O.g1_double(p) if p is not None else None for p in row]
        table.append(row)
    assert table[5][0] == O.g1_mul(g[0], 1 << 40)
    vectors = [[rnd.randrange(O.R) for _ in range(n)], [1] * n, [O.R - 1] * n, [0] * n]
    for v in vectors:
        want = None
        for s, p in zip(v, g):
            if p is not None:
                want = O.g1_add(want, O.g1_mul(p, s))
        assert shared_msm(O, table, v) == want


def _host_lib(curve):
    """tests/hosttest/hosttest_shared.cpp compiled with g++ for one curve, rebuilt when stale"""
    d = os.path.join(ROOT, "tests", "hosttest")
    src, so = os.path.join(d, "hosttest_shared.cpp"), os.path.join(d, "libhosttest_shared_%s.so" % curve)
    csrc = os.path.join(ROOT, "snark-verifier_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        flags = ["-DSNARKV_CURVE_PALLAS"] if curve == "pallas" else []
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hs_curve.restype = ctypes.c_char_p
    assert lib.hs_curve() == curve.encode()
    return lib


def _inputs(O):
    rnd = random.Random("recode-" + str(O.R % 1000))
    fixed = [0, 1, O.R - 1, (O.R - 1) // 2, (1 << 254) - 1, int.from_bytes(b"\x80" * 32, "little"),
             int.from_bytes(b"\x81" * 32, "little")]
    return fixed + [rnd.randrange(O.R) for _ in range(20000)]


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_the_recoder_of_the_device_source(curve):
    """digits in [-128, 128], no carry out of window 31, and the digits give the scalar back (values of r and above are
    brought below r first: every byte 0x80 / 0x81, and 2^254 - 1 on BN254)"""
    O = CURVES[curve]
    lib = _host_lib(curve)
    assert lib.hs_shared_recode_raw_io() == (8 << 16) | 33
    vals = _inputs(O)
    a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint32).astype(np.int64)
    a = np.ascontiguousarray(a.astype(np.uint32).view(np.int32).reshape(len(vals), 8))
    out = np.zeros((len(vals), 33), dtype=np.int32)
    lib.hs_shared_recode_raw(a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), len(vals))
    assert out[:, :32].min() >= -128 and out[:, :32].max() <= 128
    assert not out[:, 32].any()
    for v, row in zip(vals, out.tolist()):
        assert sum(d << (C_BITS * w) for w, d in enumerate(row[:32])) == v % O.R
        assert row[:32] == recode(v % O.R)[0]
