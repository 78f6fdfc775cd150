"""GPU: `Ipa::create_proof` in one call with halo2's Blake2b transcript on the device (snark_verifier_amd.ipa_create,
include/snarkv_ipa_create.h) against the oracle's `ipa_create_proof` over `Blake2bTranscript` (oracle/ipa.py,
oracle/transcript.py), byte for byte, on BN254 and pallas; against the session path (include/snarkv_ipa_prover.h) where the
Python oracle is too slow; the refusals; and the session next to it on one context."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import ipa as I  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402

pytestmark = pytest.mark.gpu
INFINITY_TEXT = "cannot write points at infinity to the transcript"


class BN:
    """BN254 as `Blake2bTranscript` takes a curve: oracle/bn254.py plus the square root its reader needs (p = 3 mod 4)"""
    R, P, B1 = O.R, O.P, O.B1
    fe_to_bytes = staticmethod(O.fe_to_bytes)
    g1_to_bytes = staticmethod(O.g1_to_bytes)

    @staticmethod
    def fq_sqrt(a):
        y = pow(a, (O.P + 1) // 4, O.P)
        return y if y * y % O.P == a % O.P else None


CURVES = {"bn254": BN, "pallas": PA}


@pytest.fixture(scope="module")
def CR():
    from snark_verifier_amd import ipa_create

    return ipa_create


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture()
def ctx_of(gpu_ctx, pctx):
    """curve name -> its context, with the oracle's IPA module switched to that curve for the test"""
    def pick(curve):
        I.use_curve(PA if curve == "pallas" else O)
        return pctx if curve == "pallas" else gpu_ctx

    yield pick
    I.use_curve(O)


def _points(curve, seed, n):
    if curve == "pallas":
        return PA.sample_points(seed, n)
    rnd = random.Random(repr(("bn-points", seed)))
    gen = O.g1_to_bytes(O.G1_GEN)
    return [O.g1_from_bytes(C.g1_mul(gen, O.fe_to_bytes(rnd.randrange(1, O.R)))) for _ in range(n)]


def _gb(curve, points):
    return b"".join(CURVES[curve].g1_to_bytes(p) for p in points)


def _dk(ctx, curve, gbytes):
    import snark_verifier_amd as sv

    return ctx.ipa_dk_create(gbytes) if curve == "pallas" else sv.IpaDecidingKey(ctx, gbytes)


class Case:
    """a key, a polynomial, an opening point and, with zk, what the reference's rng would play"""

    def __init__(self, ctx, curve, k, zk, tag):
        self.curve, self.k, self.zk, self.n = curve, k, zk, 1 << k
        r = CURVES[curve].R
        pts = _points(curve, 700 + 10 * k + zk, self.n + 2)
        self.pk = I.IpaProvingKey(k, pts[:self.n], pts[self.n], pts[self.n + 1] if zk else None)
        self.dk = _dk(ctx, curve, _gb(curve, self.pk.g))
        rnd = random.Random(repr(("create", curve, k, zk, tag)))
        self.p = [rnd.randrange(r) for _ in range(self.n)]
        self.z = rnd.randrange(r)
        self.omega = rnd.randrange(r) if zk else None
        self.p_bar = [rnd.randrange(r) for _ in range(self.n)] if zk else None
        self.omega_bar = rnd.randrange(r) if zk else None

    def oracle(self, absorbed=b"", p=None):
        """(proof bytes, (xi, U)) of oracle.ipa.ipa_create_proof; its rng replays p_bar and omega_bar"""
        t = T.Blake2bTranscript(CURVES[self.curve])
        t.state.update(absorbed)
        play = iter((self.p_bar + [self.omega_bar]) if self.zk else [])
        acc = I.ipa_create_proof(self.pk, self.p if p is None else p, self.z, self.omega, t, lambda: next(play))
        return t.finalize(), acc

    def device(self, CR, ctx, absorbed=b"", p=None):
        return CR.create_proof(ctx, self.dk, self.pk.h, self.pk.s, self.p if p is None else p, self.z, self.omega, self.p_bar,
                               self.omega_bar, absorbed)

    def close(self):
        self.dk.close()


def _session_proof(ctx, dk, curve, coeff_bytes, z, h, absorbed=b""):
    """the parent's route: the session of snarkv_ipa_prover.h driven with a hashlib Blake2b transcript (non-zk)"""
    from snark_verifier_amd import ipa_prover as P

    cv = CURVES[curve]
    t = T.Blake2bTranscript(cv)
    t.state.update(absorbed)
    xi0 = t.squeeze_challenge()
    xi = []
    with P.IpaProver(ctx, dk, coeff_bytes, z, h, xi0) as s:
        for _ in range(dk.k):
            l, r = s.round()
            for raw in (l, r):
                t.write_ec_point((int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little")))
            x = t.squeeze_challenge()
            s.fold(x)
            xi.append(x)
        u, c = s.finish()
    u = (int.from_bytes(u[:32], "little"), int.from_bytes(u[32:], "little"))
    t.write_ec_point(u)
    t.write_scalar(int.from_bytes(c, "little"))
    return t.finalize(), (xi, u)


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_oracle_parity(CR, ctx_of, curve, k, zk):
    ctx, cv = ctx_of(curve), CURVES[curve]
    c = Case(ctx, curve, k, zk, "parity")
    want_proof, want_acc = c.oracle()
    proof, acc = c.device(CR, ctx)
    assert len(proof) == CR.proof_bytes(k, zk) == 64 * k + 64 + (64 if zk else 0)
    assert proof == want_proof
    assert acc == (want_acc[0], want_acc[1])
    # the oracle's verifier reads the proof back and ends at the same accumulator, which decides
    com = c.pk.commit(c.p, c.omega)
    read = I.ipa_read_proof(zk, k, T.Blake2bTranscript(cv, proof))
    assert I.ipa_succinct_verify(c.pk.h, c.pk.s, [(1, com)], c.z, I.poly_eval(c.p, c.z), read) == acc
    assert I.ipa_decide(c.pk.g, acc)
    xib = b"".join(cv.fe_to_bytes(x) for x in acc[0])
    assert ctx.ipa_decide_batch(c.dk, xib, cv.g1_to_bytes(acc[1])) == [True]
    c.close()


def test_block_boundaries(CR, ctx_of):
    """k = 1 on pallas after every prefix length 0..130: the 128-byte boundary falls at every offset of the xi_0 squeeze, of L,
    of R and of the round's squeeze, the exactly-full buffer included"""
    ctx = ctx_of("pallas")
    c = Case(ctx, "pallas", 1, False, "blocks")
    pre = random.Random("create-prefix").randbytes(130)
    for n in range(131):
        assert c.device(CR, ctx, pre[:n]) == c.oracle(pre[:n]), n
    c.close()


def _big_key(ctx, curve, k):
    """2^k + 1 points without 2^k scalar multiplications on the host: random two-term combinations of 32 sampled points, all
    in one segmented launch"""
    n = (1 << k) + 1
    if curve == "bn254":
        return C.sample_points(14, n)
    r = PA.R
    base = PA.sample_points(14, 32)
    rnd = random.Random("big-key")
    idx = [(rnd.randrange(32), rnd.randrange(32)) for _ in range(n)]
    sc = b"".join(PA.fe_to_bytes(rnd.randrange(1, r)) for _ in range(2 * n))
    pts = b"".join(PA.g1_to_bytes(base[a]) + PA.g1_to_bytes(base[b]) for a, b in idx)
    return ctx.msm_batched(sc, pts, [2 * i for i in range(n + 1)])


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_both_msm_routes_against_the_session(CR, ctx_of, curve):
    """k = 14: the first round's MSMs have 8192 terms (Pippenger), the later ones take the segmented kernels.  Bytes equal
    those of the session driven with the hashlib transcript, from host and from device-resident coefficients."""
    import torch

    ctx, cv, k = ctx_of(curve), CURVES[curve], 14
    n = 1 << k
    gb = _big_key(ctx, curve, k)
    g, hb = gb[:64 * n], gb[64 * n:]
    assert hb != bytes(64)
    dk = _dk(ctx, curve, g)
    rnd = random.Random("k14-" + curve)
    pb = b"".join(cv.fe_to_bytes(rnd.randrange(cv.R)) for _ in range(n))
    z = rnd.randrange(cv.R)
    pre = b"k14 prefix"
    h = (int.from_bytes(hb[:32], "little"), int.from_bytes(hb[32:], "little"))
    want = _session_proof(ctx, dk, curve, pb, z, h, pre)
    assert CR.create_proof(ctx, dk, hb, None, pb, z, absorbed=pre) == want
    d_p = torch.frombuffer(bytearray(pb), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert CR.create_proof_dev(ctx, dk, hb, None, d_p.data_ptr(), n, z, absorbed=pre) == want
    xib = b"".join(cv.fe_to_bytes(x) for x in want[1][0])
    assert ctx.ipa_decide_batch(dk, xib, cv.g1_to_bytes(want[1][1])) == [True]
    dk.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_identity_is_refused_and_the_context_stays_usable(CR, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = Case(ctx, curve, 2, False, "identity")
    with pytest.raises(sv.SnarkvError) as e:
        c.device(CR, ctx, p=[0] * c.n)  # L_1 = R_1 = the identity
    assert e.value.code == sv.SNARKV_ERR_ENCODING
    assert INFINITY_TEXT in str(e.value)
    assert c.device(CR, ctx) == c.oracle()
    c.close()


def _raw_call(CR, ctx, c, pb, z, p_bar=None):
    """the C call on buffers filled with 0xAA -> (code, the buffers afterwards)"""
    a = CR.api(c.curve == "pallas")
    cap = CR.proof_bytes(c.k, True)
    bufs = [ctypes.create_string_buffer(b"\xaa" * m, m) for m in (cap, 32 * c.k, 64)]
    plen = ctypes.c_size_t(0)
    fe = lambda v: None if v is None else int(v).to_bytes(32, "little")  # noqa: E731
    pt = lambda q: None if q is None else fe(q[0]) + fe(q[1])  # noqa: E731
    rc = a.ipa_create_proof(ctx._h, c.dk._h, pt(c.pk.h), pt(c.pk.s), pb, c.n, fe(z), fe(c.omega), p_bar, fe(c.omega_bar), None, 0,
                            bufs[0], cap, ctypes.byref(plen), bufs[1], bufs[2])
    return rc, [b.raw for b in bufs]


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_validate_refuses_non_canonical_inputs_before_any_output(CR, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx, cv = ctx_of(curve), CURVES[curve]
    r = cv.R
    fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
    c, czk = Case(ctx, curve, 3, False, "validate"), Case(ctx, curve, 3, True, "validate")
    pb, pzk = b"".join(fe(v) for v in c.p), b"".join(fe(v) for v in czk.p)
    bad_coeff = pb[:32 * 5] + fe(r) + pb[32 * 6:]
    bar = b"".join(fe(v) for v in czk.p_bar)
    bad_bar = bar[:32 * 3] + fe(r) + bar[32 * 4:]
    ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
    try:
        for case, args in ((c, (bad_coeff, c.z)), (c, (pb, r)), (czk, (pzk, czk.z, bad_bar))):
            rc, bufs = _raw_call(CR, ctx, case, *args)
            assert rc == sv.SNARKV_ERR_ENCODING
            assert all(b == b"\xaa" * len(b) for b in bufs)
        rc, bufs = _raw_call(CR, ctx, czk, pzk, czk.z, bar)  # the canonical inputs pass under the flag
        assert rc == 0 and bufs[0] == czk.oracle()[0]
    finally:
        ctx.set_flags(0)
    # without the flag the call does whatever the session does with the same bytes
    for coeffs, z in ((bad_coeff, c.z), (pb, r)):
        rc, bufs = _raw_call(CR, ctx, c, coeffs, z)
        proof, (xi, u) = _session_proof(ctx, c.dk, curve, coeffs, z, c.pk.h)
        assert rc == 0
        assert bufs[0][:len(proof)] == proof
        assert bufs[1] == b"".join(fe(x) for x in xi) and bufs[2] == fe(u[0]) + fe(u[1])
    c.close()
    czk.close()


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_the_session_is_untouched(CR, ctx_of, curve):
    """a session proof after a one-call proof on the same context and key, and a one-call proof between a session's round and
    fold (the session's header allows other calls on the context between rounds): oracle bytes every time"""
    from snark_verifier_amd import ipa_prover as P

    ctx, cv = ctx_of(curve), CURVES[curve]
    c = Case(ctx, curve, 3, False, "session")
    want = c.oracle()
    pb = b"".join(cv.fe_to_bytes(v) for v in c.p)
    assert c.device(CR, ctx) == want
    assert _session_proof(ctx, c.dk, curve, pb, c.z, c.pk.h) == want
    t = T.Blake2bTranscript(cv)
    xi = []
    with P.IpaProver(ctx, c.dk, pb, c.z, c.pk.h, t.squeeze_challenge()) as s:
        for _ in range(c.k):
            l, r = s.round()
            assert c.device(CR, ctx) == want  # between round and fold
            for raw in (l, r):
                t.write_ec_point((int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little")))
            xi.append(t.squeeze_challenge())
            s.fold(xi[-1])
        u, cc = s.finish()
    u = (int.from_bytes(u[:32], "little"), int.from_bytes(u[32:], "little"))
    t.write_ec_point(u)
    t.write_scalar(int.from_bytes(cc, "little"))
    assert (t.finalize(), (xi, u)) == want
    c.close()


def test_refusals_on_a_real_context(CR, ctx_of):
    import snark_verifier_amd as sv

    ctx = ctx_of("bn254")
    c = Case(ctx, "bn254", 2, True, "refusals")
    a = CR.api(False)
    fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
    pb, bar = b"".join(fe(v) for v in c.p), b"".join(fe(v) for v in c.p_bar)
    h, s = O.g1_to_bytes(c.pk.h), O.g1_to_bytes(c.pk.s)
    out, xi, u, plen = ctypes.create_string_buffer(512), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64), ctypes.c_size_t(7)

    def call(s_, om, pbar, omb, cap=512, n=c.n):
        return a.ipa_create_proof(ctx._h, c.dk._h, h, s_, pb, n, fe(c.z), om, pbar, omb, None, 0, out, cap, ctypes.byref(plen), xi, u)

    assert call(s, fe(c.omega), bar, None) == sv.SNARKV_ERR_ARG          # a partial zk set
    assert call(None, fe(c.omega), None, None) == sv.SNARKV_ERR_ARG
    assert call(s, fe(c.omega), bar, fe(c.omega_bar), cap=255) == sv.SNARKV_ERR_LENGTH and plen.value == 256
    assert call(None, None, None, None, cap=191) == sv.SNARKV_ERR_LENGTH and plen.value == 192
    assert call(None, None, None, None, n=c.n // 2) == sv.SNARKV_ERR_LENGTH  # n is the whole key
    assert call(s, fe(c.omega), bar, fe(c.omega_bar)) == 0 and plen.value == 256
    assert out.raw[:256] == c.oracle()[0]
    c.close()


def test_product_call_in_a_child_process():
    """`snarkv_host_pallas_ipa_create_proof` at k = 3 and k = 8: the bytes of the device ABI, and an accumulator that
    `snarkv_host_pallas_ipa_decide_all` accepts (tests/ipa_create_product_child.py)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ipa_create_product_child.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "k3_equal=True k3_decides=True k8_equal=True k8_decides=True zk_equal=True", r.stdout + r.stderr
