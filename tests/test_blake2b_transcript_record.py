"""CPU: the record of the hasher's input that the host mirror's Blake2b transcript keeps for a prover
(host/blake2b_transcript.hpp: `record_absorbed`, `absorbed`, `append_opening`) -- the `absorbed` argument of
include/snarkv_ipa_multiopen.h.  After a mix of common_scalar, write_ec_point, write_scalar and squeezes, a fresh hasher over the
recorded bytes draws the challenge the transcript draws next; the bytes are the prefixes, points, scalars and the 0 byte of
each squeeze, in order, and hash to the state of the oracle's transcript; the stream is the oracle's, with the opening's bytes
appended unhashed; with the record off nothing is kept."""
import ctypes
import hashlib
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402


@pytest.fixture(scope="module")
def hook():
    import importlib.util

    from snark_verifier_amd import pallas as PL

    PL.load_library()  # HIP runtime + libsnarkv_pallas.so first
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = ctypes.CDLL(b.build_host_driver_pallas())
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    h.hp_transcript_record.argtypes = [cp, cp, sz, ctypes.c_int, cp, sz, cp, ctypes.POINTER(sz), cp, ctypes.POINTER(sz), sz, cp, cp]
    return h.hp_transcript_record


def _script(rnd, ops):
    """-> (data for the hook, the oracle's transcript after the ops, the bytes its hasher took)"""
    t, data, taken = T.Blake2bTranscript(PA), b"", b""
    pts = PA.sample_points(rnd.randrange(1 << 30), ops.count("p") + 1)
    for i, op in enumerate(ops):
        if op == "p":
            p = pts.pop()
            p = p if i % 2 else (p[0], PA.P - p[1])  # both parities of y
            t.write_ec_point(p)
            data += PA.g1_to_bytes(p)
            taken += b"\x01" + PA.g1_to_bytes(p)
        elif op == "C":
            t.squeeze_challenge()
            taken += b"\x00"
        else:
            s = rnd.choice([0, 1, PA.R - 1, rnd.randrange(PA.R)])
            (t.common_scalar if op == "s" else t.write_scalar)(s)
            data += PA.fe_to_bytes(s)
            taken += b"\x02" + PA.fe_to_bytes(s)
    return data, t, taken


@pytest.mark.parametrize("ops", ["", "C", "s", "sspppCCpCwwwwC", "spC" * 9 + "w", "p" * 5 + "C" + "w" * 12 + "CC"])
def test_the_record_hashes_to_the_transcripts_state(hook, ops):
    rnd = random.Random("record-" + ops)
    data, t, taken = _script(rnd, ops)
    tail = bytes(rnd.randrange(256) for _ in range(37))
    cap = 4096
    rec, stream, na, nb = (ctypes.create_string_buffer(n) for n in (cap, cap, 32, 32))
    rl, sl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hook(data or b"\x00", ops.encode(), len(ops), 1, tail, len(tail), rec, ctypes.byref(rl), stream, ctypes.byref(sl), cap, na, nb) == len(ops)
    assert rec.raw[:rl.value] == taken  # prefixes, points, scalars, the 0 byte of each squeeze
    assert hashlib.blake2b(taken, digest_size=64, person=b"Halo2-Transcript").digest() == t.state.copy().digest()
    assert stream.raw[:sl.value] == t.finalize() + tail  # the opening's bytes follow, and no hasher took them
    nxt = PA.fe_to_bytes(t.squeeze_challenge())
    assert na.raw == nxt and nb.raw == nxt  # the fresh hasher over the record draws the same next challenge
    # the record is opt-in: off, the transcript is as it was and keeps nothing
    assert hook(data or b"\x00", ops.encode(), len(ops), 0, tail, len(tail), rec, ctypes.byref(rl), stream, ctypes.byref(sl), cap, na, nb) == len(ops)
    assert rl.value == 0 and stream.raw[:sl.value] == t.finalize() + tail and na.raw == nxt
    assert (nb.raw == nxt) == (ops == "")  # a hasher over an empty record is a fresh transcript


def test_the_identity_is_refused_and_nothing_overflows(hook):
    rec, stream, na, nb = (ctypes.create_string_buffer(n) for n in (64, 64, 32, 32))
    rl, sl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hook(bytes(64), b"p", 1, 1, b"\x00", 0, rec, ctypes.byref(rl), stream, ctypes.byref(sl), 64, na, nb) == -10
    data = PA.g1_to_bytes(PA.G1_GEN)
    assert hook(data, b"p", 1, 1, b"\x00", 0, rec, ctypes.byref(rl), stream, ctypes.byref(sl), 64, na, nb) == -11  # 65 bytes recorded
