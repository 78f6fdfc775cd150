"""GPU: the Bgh19 multi-open prover in one call (snark_verifier_amd.ipa_multiopen, include/snarkv_ipa_multiopen.h) against
the oracle's `bgh19_create_proof` over `Blake2bTranscript` (oracle/ipa.py, oracle/transcript.py), byte for byte, on BN254 and
pallas; at k = 14, where the Python prover is too slow, against the oracle's verifier and the device's decide; a wrong
evaluation; the refusals; and `snarkv_ipa_create_proof` next to it on one context."""
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import ipa as I  # noqa: E402
import kzg as K  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402
from test_gpu_ipa_create import BN, _dk, _gb, _points  # noqa: E402
from test_ipa_multiopen_abi import multiopen_queries  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = {"bn254": BN, "pallas": PA}
MISMATCH_TEXT = "evaluation does not match the polynomial"


@pytest.fixture(scope="module")
def MO():
    from snark_verifier_amd import ipa_multiopen

    return ipa_multiopen


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture()
def ctx_of(gpu_ctx, pctx):
    """curve name -> its context, with the oracle's IPA module and the query-set grouping switched to that curve"""
    def pick(curve):
        mod = PA if curve == "pallas" else O
        I.use_curve(mod)
        K.use_curve(mod)
        return pctx if curve == "pallas" else gpu_ctx

    yield pick
    I.use_curve(O)
    K.use_curve(O)


def _fe(v):
    return int(v).to_bytes(32, "little")


class Case:
    """a zero-knowledge key, six polynomials with blinds, the query list of the issue and what the prover's rng would play"""

    def __init__(self, ctx, curve, k, tag, key_bytes=None, single_shift=False):
        self.curve, self.k, self.n = curve, k, 1 << k
        cv = CURVES[curve]
        r, n = cv.R, self.n
        rnd = random.Random(repr(("multiopen", curve, k, tag)))
        if key_bytes is None:
            pts = _points(curve, 900 + k, n + 2)
            key_bytes = _gb(curve, pts)
        else:
            pts = [(int.from_bytes(key_bytes[64 * i:64 * i + 32], "little"), int.from_bytes(key_bytes[64 * i + 32:64 * i + 64], "little"))
                   for i in range(n + 2)]
        self.pk = I.IpaProvingKey(k, pts[:n], pts[n], pts[n + 1])
        self.dk = _dk(ctx, curve, key_bytes[:64 * n])
        self.polys = [[rnd.randrange(r) for _ in range(n)] for _ in range(6)]
        self.blinds = [rnd.randrange(r) for _ in range(6)]
        self.x = rnd.randrange(1, r)
        w, w2 = rnd.randrange(2, r), rnd.randrange(2, r)
        assert w != w2
        ev = lambda poly, shift: I.poly_eval(self.polys[poly], self.x * shift % r)  # noqa: E731
        if single_shift:
            self.queries = [(p, s, ev(p, s)) for p, s in ((0, 1), (1, 1), (2, 1), (3, w))]
        else:
            self.queries = multiopen_queries(w, w2, ev)
        self.n_sets = len(K.bdfg21_query_sets(self.queries))
        self.f_blind, self.omega_bar = rnd.randrange(r), rnd.randrange(r)
        self.p_bar = [rnd.randrange(r) for _ in range(n)]
        # the commitments: the device's batched commit of the existing API, the blinds added on the host
        raw = ctx.ipa_commit_batch(self.dk, b"".join(_fe(c) for p in self.polys for c in p), n)
        self.coms = []
        for j in range(6):
            msm = (int.from_bytes(raw[64 * j:64 * j + 32], "little"), int.from_bytes(raw[64 * j + 32:64 * j + 64], "little"))
            self.coms.append(I.O.g1_add(msm, I._mul(self.pk.s, self.blinds[j])))

    def oracle(self, absorbed=b""):
        """the proof bytes of oracle.ipa.bgh19_create_proof; its rng replays f_blind, p_bar and omega_bar"""
        t = T.Blake2bTranscript(CURVES[self.curve])
        t.state.update(absorbed)
        play = iter([self.f_blind] + self.p_bar + [self.omega_bar])
        I.bgh19_create_proof(self.pk, self.polys, self.blinds, self.x, self.queries, t, lambda: next(play))
        return t.finalize()

    def device(self, MO, ctx, absorbed=b"", queries=None):
        return MO.create_proof(ctx, self.dk, self.pk.h, self.pk.s, self.polys, self.blinds, self.x,
                               self.queries if queries is None else queries, self.f_blind, self.p_bar, self.omega_bar, absorbed)

    def verify(self, proof, absorbed=b""):
        """the oracle's verifier over the proof bytes -> the accumulator (xi, U); raises when the succinct check fails"""
        t = T.Blake2bTranscript(CURVES[self.curve], proof)
        t.state.update(absorbed)
        read = I.bgh19_read_proof(self.k, self.queries, t)
        return I.bgh19_verify(self.pk.g[0], self.pk.h, self.pk.s, [K.Msm.base(c) for c in self.coms], self.x, self.queries, read)

    def decides(self, ctx, acc):
        cv = CURVES[self.curve]
        return ctx.ipa_decide_batch(self.dk, b"".join(cv.fe_to_bytes(x) for x in acc[0]), cv.g1_to_bytes(acc[1])) == [True]

    def close(self):
        self.dk.close()


def _check_parity(MO, ctx, c, absorbed=b""):
    want = c.oracle(absorbed)
    proof, acc = c.device(MO, ctx, absorbed)
    assert len(proof) == MO.proof_bytes(c.k, c.n_sets) == 64 * c.k + 32 * c.n_sets + 160
    assert proof == want
    # the oracle's verifier reads the device's bytes back and ends at the same accumulator, which the device decides
    got = c.verify(proof, absorbed)
    assert (list(got[0]), got[1]) == (acc[0], acc[1])
    assert c.decides(ctx, acc)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_oracle_parity(MO, ctx_of, curve, k):
    ctx = ctx_of(curve)
    c = Case(ctx, curve, k, "parity")
    assert c.n_sets == 3  # {0, 1, 2} at 1; {3, 4} at (1, w), 4 re-ordered; {5} at (1, w, w')
    _check_parity(MO, ctx, c)
    c.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_k1_with_single_shift_queries(MO, ctx_of, curve):
    ctx = ctx_of(curve)
    c = Case(ctx, curve, 1, "k1", single_shift=True)
    assert c.n_sets == 2
    _check_parity(MO, ctx, c)
    c.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_a_prefix_of_130_bytes(MO, ctx_of, curve):
    ctx = ctx_of(curve)
    c = Case(ctx, curve, 2, "prefix")
    _check_parity(MO, ctx, c, random.Random("multiopen-prefix").randbytes(130))
    c.close()


def _raw_call(MO, ctx, c, polys=None, blinds=None, queries=None, f_blind=None, p_bar=None, s="key", cap=None):
    """the C call on buffers filled with 0xAA -> (code, needed length, the buffers afterwards)"""
    a = MO.api(c.curve == "pallas")
    full = MO.proof_bytes(c.k, len(c.queries))
    bufs = [ctypes.create_string_buffer(b"\xaa" * m, m) for m in (full, 32 * c.k, 64)]
    plen = ctypes.c_size_t(0)
    pt = lambda q: None if q is None else _fe(q[0]) + _fe(q[1])  # noqa: E731
    pb = polys if polys is not None else b"".join(_fe(v) for p in c.polys for v in p)
    bl = blinds if blinds is not None else b"".join(_fe(v) for v in c.blinds)
    qp, qs, qe, nq = MO.pack_queries(c.queries if queries is None else queries)
    bar = p_bar if p_bar is not None else b"".join(_fe(v) for v in c.p_bar)
    rc = a.ipa_multiopen_create_proof(ctx._h, c.dk._h, pt(c.pk.h), pt(c.pk.s) if s == "key" else s, pb, c.n, 6, bl, _fe(c.x), qp, qs, qe,
                                      nq, _fe(c.f_blind) if f_blind is None else f_blind, bar, _fe(c.omega_bar), None, 0, bufs[0],
                                      full if cap is None else cap, ctypes.byref(plen), bufs[1], bufs[2])
    return rc, plen.value, [b.raw for b in bufs], a


def _untouched(bufs):
    return all(b == b"\xaa" * len(b) for b in bufs)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_a_wrong_evaluation(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx, r = ctx_of(curve), CURVES[curve].R
    c = Case(ctx, curve, 3, "wrong-eval")
    want = c.oracle()
    for at, bad_set in ((1, 0), (5, 1), (9, 2)):  # a query of each set
        bad = list(c.queries)
        bad[at] = (bad[at][0], bad[at][1], (bad[at][2] + 1) % r)
        rc, plen, bufs, a = _raw_call(MO, ctx, c, queries=bad)
        assert rc == sv.SNARKV_ERR_ARG and plen == 0
        assert MISMATCH_TEXT in a.last_error() and "set %d" % bad_set in a.last_error()
        assert _untouched(bufs)
        assert c.device(MO, ctx)[0] == want  # the next correct call on the same context
    c.close()


def _big_key_bytes(ctx, curve, k):
    """2^k + 2 points without 2^k scalar multiplications on the host (tests/test_gpu_ipa_create.py::_big_key, two spare)"""
    n = (1 << k) + 2
    if curve == "bn254":
        return C.sample_points(15, n)
    base = PA.sample_points(15, 32)
    rnd = random.Random("big-key-multiopen")
    idx = [(rnd.randrange(32), rnd.randrange(32)) for _ in range(n)]
    sc = b"".join(PA.fe_to_bytes(rnd.randrange(1, PA.R)) for _ in range(2 * n))
    pts = b"".join(PA.g1_to_bytes(base[a]) + PA.g1_to_bytes(base[b]) for a, b in idx)
    return ctx.msm_batched(sc, pts, [2 * i for i in range(n + 1)])


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_k14_against_the_verifier(MO, ctx_of, curve):
    """k = 14: the commitments of f and s and the first round take the Pippenger, the scan runs two levels.  The oracle reads
    and verifies what the device wrote from device-resident polynomials; the 2^14-term decide runs on the device."""
    import torch

    ctx, k = ctx_of(curve), 14
    c = Case(ctx, curve, k, "k14", key_bytes=_big_key_bytes(ctx, curve, k))
    d_polys = torch.frombuffer(bytearray(b"".join(_fe(v) for p in c.polys for v in p)), dtype=torch.uint8).cuda()
    d_bar = torch.frombuffer(bytearray(b"".join(_fe(v) for v in c.p_bar)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    proof, acc = MO.create_proof_dev(ctx, c.dk, c.pk.h, c.pk.s, d_polys.data_ptr(), 6, c.blinds, c.x, c.queries, c.f_blind,
                                     d_bar.data_ptr(), c.omega_bar)
    got = c.verify(proof)
    assert (list(got[0]), got[1]) == (acc[0], acc[1])
    assert c.decides(ctx, acc)
    assert c.device(MO, ctx) == (proof, acc)  # the host form gives the same bytes
    # one byte of q_eval_1 flipped: no accepted accumulator
    flipped = proof[:32] + bytes([proof[32] ^ 1]) + proof[33:]
    try:
        bad_acc = c.verify(flipped)
    except (I.IpaError, AssertionError, ValueError):
        bad_acc = None
    assert bad_acc is None or not c.decides(ctx, bad_acc)
    c.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_refusals(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx, r = ctx_of(curve), CURVES[curve].R
    c = Case(ctx, curve, 3, "refusals")
    pb = b"".join(_fe(v) for p in c.polys for v in p)
    bl = b"".join(_fe(v) for v in c.blinds)
    bar = b"".join(_fe(v) for v in c.p_bar)
    bad_shift = list(c.queries)
    bad_shift[4] = (bad_shift[4][0], r, bad_shift[4][2])
    ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
    try:
        for kw in (dict(polys=pb[:32 * 13] + _fe(r) + pb[32 * 14:]), dict(blinds=bl[:64] + _fe(r) + bl[96:]), dict(queries=bad_shift),
                   dict(f_blind=_fe(r)), dict(p_bar=bar[:32 * 3] + _fe(r) + bar[32 * 4:])):
            rc, plen, bufs, _ = _raw_call(MO, ctx, c, **kw)
            assert rc == sv.SNARKV_ERR_ENCODING and plen == 0, list(kw)
            assert _untouched(bufs)
        rc, plen, bufs, _ = _raw_call(MO, ctx, c)  # the canonical inputs pass under the flag
        assert rc == 0 and bufs[0][:plen] == c.oracle()
    finally:
        ctx.set_flags(0)
    rc, plen, bufs, _ = _raw_call(MO, ctx, c, s=None)  # the scheme is always zero-knowledge: s is required
    assert rc == sv.SNARKV_ERR_ARG and _untouched(bufs)
    need = MO.proof_bytes(3, 3)
    rc, plen, bufs, _ = _raw_call(MO, ctx, c, cap=need - 1)
    assert rc == sv.SNARKV_ERR_LENGTH and plen == need and _untouched(bufs)
    rc, plen, bufs, _ = _raw_call(MO, ctx, c, cap=need)
    assert rc == 0 and plen == need
    c.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_the_one_call_opening_is_untouched(MO, ctx_of, curve):
    """`snarkv_ipa_create_proof` (zk) before and after a multi-open proof on the same context and key: the oracle's bytes"""
    from snark_verifier_amd import ipa_create as CR

    ctx, cv = ctx_of(curve), CURVES[curve]
    c = Case(ctx, curve, 3, "next-to")
    z, omega = 12345 % cv.R, 67890 % cv.R
    t = T.Blake2bTranscript(cv)
    play = iter(c.p_bar + [c.omega_bar])
    acc = I.ipa_create_proof(c.pk, c.polys[0], z, omega, t, lambda: next(play))
    want = (t.finalize(), (list(acc[0]), acc[1]))
    one_call = lambda: CR.create_proof(ctx, c.dk, c.pk.h, c.pk.s, c.polys[0], z, omega, c.p_bar, c.omega_bar)  # noqa: E731
    assert one_call() == want
    assert c.device(MO, ctx)[0] == c.oracle()
    assert one_call() == want
    c.close()
