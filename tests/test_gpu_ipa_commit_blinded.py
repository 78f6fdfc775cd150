"""GPU: many blinded commitments against one resident IPA key (include/snarkv_ipa_commit_blinded.h; k_shared_blind of
csrc/msm_shared.hip), both curves, bit for bit against the oracle's `commit`: sizes below, at and past a slice, the blinds
where the recoding changes, a zero blind against `commit_batch_dev`, the identity as a result, a change of S on one context,
the route of one MSM per vector in a child process, and refusals that leave the output as it was."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ipa_commit_blinded_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

K = 8  # 256 bases: n = 129 is two slices of the table route


@pytest.fixture(scope="module", params=["bn254", "pallas"])
def cv(request):
    c = U.curve(request.param)
    c.gb = c.key_bytes(4242, 1 << K)
    c.key = c.dk(c.gb)
    c.s64 = c.point(0xB11D)
    yield c
    c.key.close()
    c.ctx.close()


def _blinds(cv, rnd):
    """zero, one, r - 1, every byte 0x80 (the recoding's carry chain; above r, it counts mod r), a random one"""
    return [0, 1, cv.R - 1, int.from_bytes(b"\x80" * 32, "little"), rnd.randrange(cv.R)]


def _plain(cv, vecs):
    import torch

    n, m = len(vecs[0]), len(vecs)
    d_in = torch.frombuffer(bytearray(b"".join(U.enc(v) for v in vecs)), dtype=torch.uint8).cuda()
    d_out = torch.zeros(64 * m, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cv.ctx.ipa_commit_batch_dev(cv.key, d_in.data_ptr(), n, m, d_out.data_ptr(), 0)
    cv.ctx.sync()
    return bytes(d_out.cpu().numpy())


@pytest.mark.parametrize("n", [1, 7, 8, 129])
def test_five_vectors_with_the_five_blinds(cv, n):
    rnd = random.Random("cbb-5-%d" % n)
    vecs = [[rnd.randrange(cv.R) for _ in range(n)] for _ in range(5)]
    blinds = _blinds(cv, rnd)
    got = U.run(cv, cv.key, cv.s64, vecs, blinds)
    for a in range(5):
        assert got[64 * a:64 * a + 64] == U.expected(cv, cv.gb, cv.s64, vecs[a], blinds[a]), (cv.name, n, a)
    assert got[:64] == _plain(cv, vecs)[:64]  # the zero blind: the bytes of commit_batch_dev


@pytest.mark.parametrize("n", [1, 7, 8, 129])
def test_one_vector_with_each_blind(cv, n):
    rnd = random.Random("cbb-1-%d" % n)
    vec = [rnd.randrange(cv.R) for _ in range(n)]
    plain = _plain(cv, [vec])
    for b in _blinds(cv, rnd):
        got = U.run(cv, cv.key, cv.s64, [vec], [b])
        assert got == U.expected(cv, cv.gb, cv.s64, vec, b), (cv.name, n, hex(b))
        if b == 0:
            assert got == plain


@pytest.mark.parametrize("slices", [1, 3])
def test_forced_slices(cv, slices):
    """the blind's partial sits after the slices' whatever their number"""
    rnd = random.Random("cbb-slices")
    vecs = [[rnd.randrange(cv.R) for _ in range(129)] for _ in range(2)]
    blinds = [rnd.randrange(cv.R), cv.R - 1]
    got = U.run(cv, cv.key, cv.s64, vecs, blinds, slices)
    for a in range(2):
        assert got[64 * a:64 * a + 64] == U.expected(cv, cv.gb, cv.s64, vecs[a], blinds[a])


def test_the_blind_term_cancels_the_commitment(cv):
    """S = -G[0] and poly = (blind, 0, ...): the sum is the identity, 64 zero bytes; beside it a vector that does not cancel"""
    rnd = random.Random("cbb-cancel")
    s64 = cv.neg(cv.gb[:64])
    for b in (1, cv.R - 1, rnd.randrange(cv.R)):
        other = [rnd.randrange(cv.R) for _ in range(8)]
        got = U.run(cv, cv.key, s64, [[b] + [0] * 7, other], [b, b])
        assert got[:64] == bytes(64)
        assert got[64:] == U.expected(cv, cv.gb, s64, other, b)


def test_s_changes_between_calls_on_one_context(cv):
    """the rows 2^(8 w) S stay with the context: a new S rebuilds them, the old S again rebuilds them again"""
    rnd = random.Random("cbb-s")
    vec, b = [rnd.randrange(cv.R) for _ in range(7)], rnd.randrange(cv.R)
    s1, s2 = cv.s64, cv.point(0xC0FFEE)
    for s64 in (s1, s2, s2, s1):
        assert U.run(cv, cv.key, s64, [vec], [b]) == U.expected(cv, cv.gb, s64, vec, b)
    ctx = cv.new_ctx()  # a second context on the same key has rows of its own
    try:
        assert U.run(cv, cv.key, s2, [vec], [b], ctx=ctx) == U.expected(cv, cv.gb, s2, vec, b)
        assert U.run(cv, cv.key, s1, [vec], [b]) == U.expected(cv, cv.gb, s1, vec, b)
    finally:
        ctx.close()


def test_refusals_leave_the_output_untouched(cv):
    import snark_verifier_amd as sv

    rnd = random.Random("cbb-refuse")
    vecs = [[rnd.randrange(cv.R) for _ in range(8)] for _ in range(2)]
    blinds = [rnd.randrange(cv.R), rnd.randrange(cv.R)]
    untouched = bytes([U.FILL]) * 128
    off_curve = (1).to_bytes(32, "little") * 2  # (1, 1): 1 != 1 + b on either curve
    big_x = ((1 << 256) - 1).to_bytes(32, "little") + cv.s64[32:]
    ctx = cv.new_ctx()
    try:
        def refused(code, s64, vs, bs, c=ctx):
            with pytest.raises(sv.SnarkvError) as e:
                U.run(cv, cv.key, s64, vs, bs, ctx=c)
            assert e.value.code == code, e.value
            assert U.run.last_out == untouched[:64 * len(vs)]

        refused(sv.SNARKV_ERR_ARG, cv.s64, vecs, None)
        refused(sv.SNARKV_ERR_ARG, None, vecs, blinds)
        refused(sv.SNARKV_ERR_ENCODING, bytes(64), vecs, blinds)              # S at infinity, flag or no flag
        refused(sv.SNARKV_ERR_LENGTH, cv.s64, [[1] * ((1 << K) + 1)], [1])    # n > 2^k
        ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
        assert U.run(cv, cv.key, cv.s64, vecs, blinds, ctx=ctx) == b"".join(
            U.expected(cv, cv.gb, cv.s64, v, b) for v, b in zip(vecs, blinds))
        refused(sv.SNARKV_ERR_ENCODING, cv.s64, vecs, [blinds[0], cv.R])      # a blind that is not canonical
        refused(sv.SNARKV_ERR_ENCODING, off_curve, vecs, blinds)
        refused(sv.SNARKV_ERR_ENCODING, big_x, vecs, blinds)
        refused(sv.SNARKV_ERR_ENCODING, cv.s64, [vecs[0], vecs[1][:7] + [cv.R]], blinds)  # a coefficient that is not
        ctx.set_flags(0)  # without the flag a blind counts mod r
        got = U.run(cv, cv.key, cv.s64, vecs, [blinds[0], cv.R + 5], ctx=ctx)
        assert got[64:] == U.expected(cv, cv.gb, cv.s64, vecs[1], 5)
    finally:
        ctx.close()


def test_the_per_vector_route_in_a_child_process():
    """SNARKV_IPA_SHARED=0 is read once per process: a fresh child, both curves in it"""
    script = os.path.join(ROOT, "tests", "ipa_commit_blinded_child.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, SNARKV_IPA_SHARED="0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "per-vector ok" in r.stdout, r.stdout + r.stderr
