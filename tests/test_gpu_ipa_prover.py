"""GPU: the IPA prover on the device (snark_verifier_amd.ipa_prover, include/snarkv_ipa_prover.h) against the
oracle's `ipa_create_proof` / `ipa_as_create_proof` (oracle/ipa.py), byte for byte, on BN254 and pallas; the
fold edge cases through the session; and misuse of the session."""
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
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402
from ipa_util import pack_acc, pack_svk  # noqa: E402

pytestmark = pytest.mark.gpu
TR = {"evm": (0, T.EvmTranscript), "poseidon": (1, T.PoseidonTranscript)}


@pytest.fixture(scope="module")
def P():
    from snark_verifier_amd import ipa_prover

    return ipa_prover


@pytest.fixture(scope="module")
def H():
    from hostfmt import load_host_lib

    h = load_host_lib()
    cp, u32, sz = ctypes.c_char_p, ctypes.c_uint32, ctypes.c_size_t
    h.hd_ipa_succinct_verify.argtypes = [ctypes.c_int, cp, cp, cp, cp, cp, sz, cp]
    h.hd_ipa_decide_all.argtypes = [u32, cp, sz, cp, u32]
    h.hd_ipa_create_proof.argtypes = [ctypes.c_int, cp, cp, sz, cp, cp, cp, cp, sz, cp, sz, ctypes.POINTER(sz), cp]
    h.hd_ipa_as_create_proof.argtypes = [ctypes.c_int, cp, cp, sz, cp, u32, cp, sz, cp, sz, ctypes.POINTER(sz), cp]
    return h


class _Recorder:
    """a seeded rng that records what it plays (the host mirror takes the same scalars as a list)"""

    def __init__(self, seed, r):
        self.rnd, self.r, self.played = random.Random(repr(seed)), r, []

    def __call__(self):
        v = self.rnd.randrange(self.r)
        self.played.append(v)
        return v


def _host_prove(fn, tkind, args, k, played, mod=O):
    cap = 1 << 16
    proof, plen, acc = ctypes.create_string_buffer(cap), ctypes.c_size_t(0), ctypes.create_string_buffer(32 * k + 64)
    rb = b"".join(mod.fe_to_bytes(v) for v in played)
    rc = fn(tkind, *args, rb or b"\x00", len(played), proof, cap, ctypes.byref(plen), acc)
    assert rc == 1, rc
    return proof.raw[:plen.value], acc.raw


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture()
def on_pallas():
    I.use_curve(PA)
    yield
    I.use_curve(O)


def _bn_points(seed, n):
    rnd = random.Random(repr(seed))
    gen = O.g1_to_bytes(O.G1_GEN)
    return [O.g1_from_bytes(C.g1_mul(gen, O.fe_to_bytes(rnd.randrange(1, O.R)))) for _ in range(n)]


def _bn_key(seed, k, zk):
    pts = _bn_points(seed, (1 << k) + 2)
    n = 1 << k
    return I.IpaProvingKey(k, pts[:n], pts[n], pts[n + 1] if zk else None)


def _gb(points, mod=O):
    return b"".join(mod.g1_to_bytes(p) for p in points)


def _rng(seed, r):
    rnd = random.Random(repr(seed))
    return lambda: rnd.randrange(r)


@pytest.mark.parametrize("tr", ["evm", "poseidon"])
@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("k", [1, 2, 5, 10])
def test_create_proof_byte_exact_bn254(P, H, gpu_ctx, k, zk, tr):
    import snark_verifier_amd as sv

    tk, Tr = TR[tr]
    pk = _bn_key(("key", k, zk), k, zk)
    dk = sv.IpaDecidingKey(gpu_ctx, _gb(pk.g))
    seed = ("prove", k, zk, tr)
    rnd = random.Random(repr(seed))
    n = 1 << k
    p = [rnd.randrange(O.R) for _ in range(n)]
    z = rnd.randrange(O.R)
    omega = rnd.randrange(O.R) if zk else None
    want_t = Tr()
    want = I.ipa_create_proof(pk, p, z, omega, want_t, _rng(seed + ("rng",), O.R))
    got_t = Tr()
    got = P.create_proof(gpu_ctx, dk, pk.h, pk.s, p, z, omega, got_t, _rng(seed + ("rng",), O.R))
    assert got_t.finalize() == want_t.finalize()
    assert pack_acc(got) == pack_acc(want)
    # the host mirror accepts the proof and decides the accumulator
    proof = got_t.finalize()
    com = O.g1_to_bytes(pk.commit(p, omega))
    svk = pack_svk(k, pk.g[0], pk.h, pk.s)
    out = ctypes.create_string_buffer(32 * k + 64)
    ev = O.fe_to_bytes(I.poly_eval(p, z))
    assert H.hd_ipa_succinct_verify(tk, svk, com, O.fe_to_bytes(z), ev, proof, len(proof), out) == 1
    assert out.raw == pack_acc(got)
    assert H.hd_ipa_decide_all(k, _gb(pk.g), n, out.raw, 1) == 1
    # the host mirror's Ipa::create_proof drives the same session: byte-exact too
    rec = _Recorder(seed + ("rng",), O.R)
    I.ipa_create_proof(pk, p, z, omega, Tr(), rec)
    pb = b"".join(O.fe_to_bytes(c) for c in p)
    om = O.fe_to_bytes(omega) if zk else None
    hp, hacc = _host_prove(H.hd_ipa_create_proof, tk, (svk, _gb(pk.g), n, pb, O.fe_to_bytes(z), om), k, rec.played)
    assert hp == proof
    assert hacc == pack_acc(got)
    dk.close()


@pytest.mark.parametrize("zk", [False, True])
@pytest.mark.parametrize("m", [2, 10])
def test_as_create_proof_byte_exact_bn254(P, H, gpu_ctx, m, zk):
    import snark_verifier_amd as sv

    k = 5
    pk = _bn_key(("askey", zk), k, zk)
    dk = sv.IpaDecidingKey(gpu_ctx, _gb(pk.g))
    rnd = random.Random(repr(("accs", m, zk)))
    accs = [([rnd.randrange(O.R) for _ in range(k)], None) for _ in range(m)]
    accs = [(xi, I._msm(I.h_coeffs(xi, 1), pk.g)) for xi, _ in accs]  # accumulators that decide
    seed = ("as", m, zk)
    want_t, got_t = T.EvmTranscript(), T.EvmTranscript()
    want = I.ipa_as_create_proof(pk, accs, want_t, _rng(seed, O.R))
    got = P.as_create_proof(gpu_ctx, dk, pk.h, pk.s, accs, got_t, _rng(seed, O.R))
    assert got_t.finalize() == want_t.finalize()
    assert pack_acc(got) == pack_acc(want)
    proof = I.ipa_as_read_proof(zk, k, accs, T.EvmTranscript(got_t.finalize()))
    new = I.ipa_as_verify(pk.h, pk.s, accs, proof)
    assert gpu_ctx.ipa_decide_batch(dk, b"".join(O.fe_to_bytes(x) for x in new[0]), O.g1_to_bytes(new[1])) == [True]
    # the host mirror's IpaAs::create_proof
    rec = _Recorder(seed, O.R)
    I.ipa_as_create_proof(pk, accs, T.EvmTranscript(), rec)
    accb = b"".join(pack_acc(a) for a in accs)
    svk = pack_svk(k, pk.g[0], pk.h, pk.s)
    hp, hacc = _host_prove(H.hd_ipa_as_create_proof, 0, (svk, _gb(pk.g), 1 << k, accb, m), k, rec.played)
    assert hp == got_t.finalize()
    assert hacc == pack_acc(got)
    dk.close()


@pytest.mark.parametrize("zk", [False, True])
def test_as_combine_against_the_oracle(P, gpu_ctx, zk):
    import torch

    rnd = random.Random(repr(("combine", zk)))
    for k, m in ((1, 1), (4, 3), (9, 10)):
        xis = [[rnd.randrange(O.R) for _ in range(k)] for _ in range(m)]
        alpha = rnd.randrange(O.R)
        ab = (rnd.randrange(O.R), rnd.randrange(O.R)) if zk else None
        hs = [I.h_coeffs(xi, 1) for xi in xis]
        if ab:
            hs.append([ab[1], ab[0]] + [0] * ((1 << k) - 2))
        want = [sum(pow(alpha, i, O.R) * hc[j] for i, hc in enumerate(hs)) % O.R for j in range(1 << k)]
        d_h = torch.empty(32 << k, dtype=torch.uint8, device="cuda")
        P.as_combine_dev(gpu_ctx, xis, alpha, ab, d_h.data_ptr())
        assert d_h.cpu().numpy().tobytes() == b"".join(O.fe_to_bytes(x) for x in want)


@pytest.mark.parametrize("zk", [False, True])
def test_reference_test_ipa_on_pallas(P, pctx, on_pallas, zk):
    """`test_ipa` (pcs/ipa.rs:434-466): k = 10, Blake2b, pallas."""
    k, n = 10, 1 << 10
    pts = PA.sample_points(300 + zk, n + 2)
    pk = I.IpaProvingKey(k, pts[:n], pts[n], pts[n + 1] if zk else None)
    dk = pctx.ipa_dk_create(_gb(pk.g, PA))
    rnd = random.Random(repr(("pallas", zk)))
    p = [rnd.randrange(PA.R) for _ in range(n)]
    z = rnd.randrange(PA.R)
    omega = rnd.randrange(PA.R) if zk else None
    want_t, got_t = T.Blake2bTranscript(PA), T.Blake2bTranscript(PA)
    want = I.ipa_create_proof(pk, p, z, omega, want_t, _rng(("pr", zk), PA.R))
    got = P.create_proof(pctx, dk, pk.h, pk.s, p, z, omega, got_t, _rng(("pr", zk), PA.R))
    assert got_t.finalize() == want_t.finalize()
    assert got == want
    c = pk.commit(p, omega)
    acc = I.ipa_succinct_verify(pk.h, pk.s, [(1, c)], z, I.poly_eval(p, z),
                                I.ipa_read_proof(zk, k, T.Blake2bTranscript(PA, got_t.finalize())))
    assert acc == got
    xi = b"".join(PA.fe_to_bytes(x) for x in acc[0])
    assert pctx.ipa_decide_batch(dk, xi, PA.g1_to_bytes(acc[1])) == [True]
    # the pasta flavour of the host mirror (hp_ipa_create_proof, Blake2b)
    hpl = _pallas_host()
    rec = _Recorder(("pr", zk), PA.R)
    I.ipa_create_proof(pk, p, z, omega, T.Blake2bTranscript(PA), rec)
    svk = _pack_svk_pallas(k, pk.g[0], pk.h, pk.s)
    pb = b"".join(PA.fe_to_bytes(c) for c in p)
    om = PA.fe_to_bytes(omega) if zk else None
    hp, hacc = _host_prove(hpl.hp_ipa_create_proof, 0, (svk, _gb(pk.g, PA), n, pb, PA.fe_to_bytes(z), om), k, rec.played, PA)
    assert hp == got_t.finalize()
    assert hacc == b"".join(PA.fe_to_bytes(x) for x in got[0]) + PA.g1_to_bytes(got[1])
    dk.close()


def _pack_svk_pallas(k, g0, h, s):
    import struct

    return struct.pack("<II", k, 1 if s is not None else 0) + PA.g1_to_bytes(g0) + PA.g1_to_bytes(h) + (
        PA.g1_to_bytes(s) if s is not None else b"")


def _pallas_host():
    import importlib.util

    import snark_verifier_amd as sv

    sv.load_library()
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = ctypes.CDLL(b.build_host_driver_pallas())
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    h.hp_ipa_create_proof.argtypes = [ctypes.c_int, cp, cp, sz, cp, cp, cp, cp, sz, cp, sz, ctypes.POINTER(sz), cp]
    return h


def test_reference_test_ipa_as_on_pallas(P, pctx, on_pallas):
    """`test_ipa_as` (accumulation.rs:240-290): k = 10, zk, m = 10, Blake2b, pallas."""
    k, n, m = 10, 1 << 10, 10
    pts = PA.sample_points(400, n + 2)
    pk = I.IpaProvingKey(k, pts[:n], pts[n], pts[n + 1])
    dk = pctx.ipa_dk_create(_gb(pk.g, PA))
    rnd = random.Random("pallas-as")
    rng = lambda: rnd.randrange(PA.R)  # noqa: E731
    accs = []
    for _ in range(m):  # the input accumulators come from the device prover itself
        p = [rng() for _ in range(n)]
        omega, z = rng(), rng()
        t = T.Blake2bTranscript(PA)
        accs.append(P.create_proof(pctx, dk, pk.h, pk.s, p, z, omega, t, rng))
    want_t, got_t = T.Blake2bTranscript(PA), T.Blake2bTranscript(PA)
    want = I.ipa_as_create_proof(pk, accs, want_t, _rng("pas", PA.R))
    got = P.as_create_proof(pctx, dk, pk.h, pk.s, accs, got_t, _rng("pas", PA.R))
    assert got_t.finalize() == want_t.finalize()
    assert got == want
    new = I.ipa_as_verify(pk.h, pk.s, accs, I.ipa_as_read_proof(True, k, accs, T.Blake2bTranscript(PA, got_t.finalize())))
    everything = accs + [new]
    xi = b"".join(PA.fe_to_bytes(x) for a in everything for x in a[0])
    u = b"".join(PA.g1_to_bytes(a[1]) for a in everything)
    assert pctx.ipa_decide_batch(dk, xi, u) == [True] * (m + 1)
    dk.close()


def _model_rounds(g, p, z, h, xi0, xis):
    """the oracle's prover loop with the challenges given: [(L, R)], U, c"""
    n = len(g)
    hp = I._mul(h, xi0)
    bases, coeffs, zs = list(g), [c % O.R for c in p], [pow(z, i, O.R) for i in range(n)]
    out = []
    for x in xis:
        half = len(bases) // 2
        l = O.g1_add(I._msm(coeffs[half:], bases[:half]), I._mul(hp, I.inner_product(coeffs[half:], zs[:half])))
        r = O.g1_add(I._msm(coeffs[:half], bases[half:]), I._mul(hp, I.inner_product(coeffs[:half], zs[half:])))
        out.append((l, r))
        xinv = pow(x, O.R - 2, O.R)
        bases = [O.g1_add(bases[j], I._mul(bases[half + j], x)) for j in range(half)]
        coeffs = [(coeffs[j] + xinv * coeffs[half + j]) % O.R for j in range(half)]
        zs = [(zs[j] + x * zs[half + j]) % O.R for j in range(half)]
    return out, bases[0], coeffs[0]


def _session(P, ctx, dk, g, p, z, h, xi0, xis):
    got = []
    with P.IpaProver(ctx, dk, b"".join(O.fe_to_bytes(c) for c in p), z, h, xi0) as s:
        for x in xis:
            l, r = s.round()
            got.append((O.g1_from_bytes(l), O.g1_from_bytes(r)))
            s.fold(x)
        u, c = s.finish()
    return got, O.g1_from_bytes(u), O.fe_from_bytes(c)


@pytest.mark.parametrize("case", ["random", "xi0", "xi1", "xi_minus1", "opposite", "equal", "identity"])
def test_fold_edge_cases(P, gpu_ctx, case):
    import snark_verifier_amd as sv

    k = 3 if case != "random" else 10
    n, half = 1 << k, 1 << (k - 1)
    g = _bn_points(("edge", case), n)
    rx = random.Random(repr(("edge-xi", case)))
    xis = {"xi0": [0] * k, "xi1": [1] * k, "xi_minus1": [O.R - 1] * k,
           "random": [rx.randrange(O.R) for _ in range(k)]}.get(case, [1] * k)
    if case == "opposite":
        g[:half] = [O.g1_neg(q) for q in g[half:]]
    elif case == "equal":
        g[:half] = list(g[half:])
    elif case == "identity":
        g[1] = g[half + 2] = None
    rnd = random.Random(repr(("edge-s", case)))
    p = [rnd.randrange(O.R) for _ in range(n)]
    z, xi0 = rnd.randrange(O.R), rnd.randrange(1, O.R)
    h = _bn_points(("edge-h", case), 1)[0]
    dk = sv.IpaDecidingKey(gpu_ctx, _gb(g))
    assert _session(P, gpu_ctx, dk, g, p, z, h, xi0, xis) == _model_rounds(g, p, z, h, xi0, xis)
    dk.close()


def test_large_k16_byte_exact(P, gpu_ctx):
    import snark_verifier_amd as sv

    k = 16
    pk = _bn_key("k16", k, False)
    dk = sv.IpaDecidingKey(gpu_ctx, _gb(pk.g))
    rnd = random.Random("k16p")
    p = [rnd.randrange(O.R) for _ in range(1 << k)]
    z = rnd.randrange(O.R)
    want_t, got_t = T.EvmTranscript(), T.EvmTranscript()
    want = I.ipa_create_proof(pk, p, z, None, want_t, None)
    got = P.create_proof(gpu_ctx, dk, pk.h, None, p, z, None, got_t, None)
    assert got_t.finalize() == want_t.finalize()
    assert got == want
    dk.close()


def test_large_k20_verifies_and_decides(P, gpu_ctx):
    import torch
    import snark_verifier_amd as sv

    k = 20
    n = 1 << k
    d = torch.empty(64 * (n + 1), dtype=torch.uint8, device="cuda")
    gpu_ctx.sample_points_dev(20, n + 1, d.data_ptr())
    gpu_ctx.sync()
    gb = d.cpu().numpy().tobytes()
    g0, h = O.g1_from_bytes(gb[:64]), O.g1_from_bytes(gb[64 * n:])
    dk = sv.IpaDecidingKey(gpu_ctx, gb[:64 * n])
    rnd = random.Random("k20")
    p = [rnd.randrange(O.R) for _ in range(n)]
    z = rnd.randrange(O.R)
    t = T.PoseidonTranscript()
    xi, u = P.create_proof(gpu_ctx, dk, h, None, p, z, None, t, None)
    c = P.commit(gpu_ctx, dk, p)
    acc = I.ipa_succinct_verify(h, None, [(1, c)], z, I.poly_eval(p, z),
                                I.ipa_read_proof(False, k, T.PoseidonTranscript(t.finalize())))
    assert acc == (xi, u)
    assert g0 is not None
    assert gpu_ctx.ipa_decide_batch(dk, b"".join(O.fe_to_bytes(x) for x in xi), O.g1_to_bytes(u)) == [True]
    dk.close()


def test_misuse_and_interleaved_calls(P, gpu_ctx):
    import snark_verifier_amd as sv

    k = 4
    n = 1 << k
    pk = _bn_key("misuse", k, False)
    dk = sv.IpaDecidingKey(gpu_ctx, _gb(pk.g))
    rnd = random.Random("misuse")
    p = [rnd.randrange(O.R) for _ in range(n)]
    pb = b"".join(O.fe_to_bytes(c) for c in p)
    z, xi0 = rnd.randrange(O.R), rnd.randrange(O.R)
    xis = [rnd.randrange(1, O.R) for _ in range(k)]
    want = _model_rounds(pk.g, p, z, pk.h, xi0, xis)

    def code(fn, *a):
        with pytest.raises(sv.SnarkvError) as e:
            fn(*a)
        return e.value.code

    assert code(P.IpaProver, gpu_ctx, dk, pb[:-32], z, pk.h, xi0) == sv.SNARKV_ERR_LENGTH
    with P.IpaProver(gpu_ctx, dk, pb, z, pk.h, xi0) as s:
        assert code(s.fold, xis[0]) == sv.SNARKV_ERR_ARG      # fold before round
        assert code(s.finish) == sv.SNARKV_ERR_ARG            # finish before round k
        got = []
        for i, x in enumerate(xis):
            l, r = s.round()
            assert code(s.round) == sv.SNARKV_ERR_ARG         # two rounds without a fold
            got.append((O.g1_from_bytes(l), O.g1_from_bytes(r)))
            # other work on the same context between the rounds
            gpu_ctx.msm_pippenger(pb, _gb(pk.g))
            assert gpu_ctx.ipa_decide_batch(dk, b"".join(O.fe_to_bytes(v) for v in xis), O.g1_to_bytes(pk.h)) == [False]
            s.fold(x)
        assert code(s.round) == sv.SNARKV_ERR_ARG             # a (k+1)-th round
        u, c = s.finish()
    assert (got, O.g1_from_bytes(u), O.fe_from_bytes(c)) == want
    # SNARKV_FLAG_VALIDATE: non-canonical scalars are refused
    gpu_ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
    try:
        bad = O.fe_to_bytes(O.R) + pb[32:]
        assert code(P.IpaProver, gpu_ctx, dk, bad, z, pk.h, xi0) == sv.SNARKV_ERR_ENCODING
        with P.IpaProver(gpu_ctx, dk, pb, z, pk.h, xi0) as s:
            s.round()
            assert code(s.fold, O.fe_to_bytes(O.R)) == sv.SNARKV_ERR_ENCODING
    finally:
        gpu_ctx.set_flags(0)
    dk.close()
