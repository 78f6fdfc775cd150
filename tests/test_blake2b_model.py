"""CPU: the Blake2b transcript the device compiles (snark-verifier_amd/csrc/blake2b_dev.h), run on the host through
tests/hosttest/hosttest_blake2b.cpp for both curves: the hash against hashlib at every length and every split of an
update, the reduction of a digest mod r (`from_uniform_bytes`) against Python integers at the edges of both fields, point
compression, and a scripted transcript against oracle/transcript.py's `Blake2bTranscript`."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402

CURVES = {"bn254": BN, "pallas": PA}
PERSON = b"Halo2-Transcript"
_LIBS = {}


def _host_lib(curve):
    """tests/hosttest/hosttest_blake2b.cpp compiled with g++ for one curve, rebuilt when stale"""
    if curve in _LIBS:
        return _LIBS[curve]
    d = os.path.join(ROOT, "tests", "hosttest")
    src, so = os.path.join(d, "hosttest_blake2b.cpp"), os.path.join(d, "libhosttest_blake2b_%s.so" % curve)
    csrc = os.path.join(ROOT, "snark-verifier_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        flags = ["-DSNARKV_CURVE_PALLAS"] if curve == "pallas" else []
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hb_curve.restype = ctypes.c_char_p
    assert lib.hb_curve() == curve.encode()
    sz, cp = ctypes.c_size_t, ctypes.c_char_p
    lib.hb_digest_split.argtypes = [cp, sz, sz, cp]
    lib.hb_tr_update.argtypes = [cp, cp, sz]
    _LIBS[curve] = lib
    return lib


def _digest(lib, msg, cut=0):
    out = ctypes.create_string_buffer(64)
    lib.hb_digest_split(msg if msg else b"\x00", len(msg), cut, out)
    return out.raw


def _reduce(lib, digest):
    out = ctypes.create_string_buffer(32)
    lib.hb_reduce(digest, out)
    return int.from_bytes(out.raw, "little")


def test_digest_matches_hashlib_at_every_length():
    lib = _host_lib("pallas")  # the hash does not depend on the curve
    rnd = random.Random("blake2b-lengths")
    for n in range(261):
        msg = rnd.randbytes(n)
        assert _digest(lib, msg) == hashlib.blake2b(msg, digest_size=64, person=PERSON).digest(), n


def test_incremental_updates_split_at_every_position():
    lib = _host_lib("bn254")
    msg = random.Random("blake2b-splits").randbytes(200)
    want = hashlib.blake2b(msg, digest_size=64, person=PERSON).digest()
    for cut in range(201):
        assert _digest(lib, msg, cut) == want, cut


def test_state_keeps_absorbing_after_a_digest():
    """the digest is of a copy: a squeeze in the middle does not disturb what follows, the exactly-full buffer included"""
    lib = _host_lib("pallas")
    msg = random.Random("blake2b-copy").randbytes(300)
    for first in (0, 1, 127, 128, 129, 256):
        st = ctypes.create_string_buffer(lib.hb_state_bytes())
        lib.hb_tr_init(st)
        lib.hb_tr_update(st, msg, first)
        out = ctypes.create_string_buffer(32)
        lib.hb_tr_squeeze(st, out)
        lib.hb_tr_update(st, msg[first:], len(msg) - first)
        lib.hb_tr_squeeze(st, out)
        h = hashlib.blake2b(msg[:first] + b"\x00" + msg[first:] + b"\x00", digest_size=64, person=PERSON).digest()
        assert int.from_bytes(out.raw, "little") == int.from_bytes(h, "little") % PA.R, first


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_squeeze_reduction_is_exact(curve):
    lib, r = _host_lib(curve), CURVES[curve].R
    top = (1 << 256) - 1
    cases = [(0, 0), (top, top)]
    cases += [(lo, 0) for lo in (r - 1, r, r + 1, top)]
    cases += [(0, hi) for hi in (1, r - 1, top)]
    for lo, hi in cases:
        d = lo.to_bytes(32, "little") + hi.to_bytes(32, "little")
        assert _reduce(lib, d) == (lo + (hi << 256)) % r, (hex(lo), hex(hi))
    rnd = random.Random("blake2b-reduce-" + curve)
    for _ in range(1000):
        d = rnd.randbytes(64)
        assert _reduce(lib, d) == int.from_bytes(d, "little") % r


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_compress_point_on_both_parities(curve):
    lib, C = _host_lib(curve), CURVES[curve]
    pts = PA.sample_points(11, 8) if curve == "pallas" else [BN.g1_mul(BN.G1_GEN, 3 + i) for i in range(8)]
    pts += [C.g1_neg(p) for p in pts]
    assert {p[1] & 1 for p in pts} == {0, 1}
    for x, y in pts:
        out = ctypes.create_string_buffer(32)
        lib.hb_compress_point(C.fe_to_bytes(x), C.fe_to_bytes(y), out)
        assert out.raw == (x | ((y & 1) << 255)).to_bytes(32, "little")


def _points(curve, n):
    return PA.sample_points(12, n) if curve == "pallas" else [BN.g1_mul(BN.G1_GEN, 5 + i) for i in range(n)]


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_scripted_transcript_agrees_with_the_oracle(curve):
    """point, point, squeeze, scalar, squeeze, squeeze -- challenge by challenge"""
    lib, C = _host_lib(curve), CURVES[curve]
    p0, p1 = _points(curve, 2)
    o = T.Blake2bTranscript(C)
    st = ctypes.create_string_buffer(lib.hb_state_bytes())
    lib.hb_tr_init(st)
    out = ctypes.create_string_buffer(32)

    def squeeze():
        lib.hb_tr_squeeze(st, out)
        assert int.from_bytes(out.raw, "little") == o.squeeze_challenge()
        return int.from_bytes(out.raw, "little")

    for p in (p0, p1):
        o.common_ec_point(p)
        assert lib.hb_tr_common_point(st, C.fe_to_bytes(p[0]), C.fe_to_bytes(p[1])) == 1
    c = squeeze()
    o.common_scalar(c)
    lib.hb_tr_common_scalar(st, C.fe_to_bytes(c))
    squeeze()
    squeeze()
    # the identity is refused and nothing is absorbed
    assert lib.hb_tr_common_point(st, bytes(32), bytes(32)) == 0
    squeeze()


@pytest.mark.parametrize("curve", sorted(CURVES))
def test_round_message_at_every_block_offset(curve):
    """the round kernel's shape (two points and the challenge's prefix as ONE message) after every prefix length 0..130"""
    lib, C = _host_lib(curve), CURVES[curve]
    l, r = _points(curve, 2)
    lr = C.fe_to_bytes(l[0]) + C.fe_to_bytes(l[1]) + C.fe_to_bytes(r[0]) + C.fe_to_bytes(r[1])
    pre = random.Random("blake2b-round").randbytes(130)
    for n in range(131):
        o = T.Blake2bTranscript(C)
        o.state.update(pre[:n])
        o.write_ec_point(l)
        o.write_ec_point(r)
        st = ctypes.create_string_buffer(lib.hb_state_bytes())
        lib.hb_tr_init(st)
        lib.hb_tr_update(st, pre, n)
        proof, xi = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        assert lib.hb_tr_round(st, lr, proof, xi) == 1
        assert proof.raw == o.finalize()
        assert int.from_bytes(xi.raw, "little") == o.squeeze_challenge(), n
