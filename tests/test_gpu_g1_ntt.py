"""GPU: the transform over group elements (snark_verifier_amd.g1_ntt, include/snarkv_g1_ntt.h) on BN254 and pallas against
the reference of tests/g1_ntt_util.py (a bit-reversal radix-2 transform on the oracle's point arithmetic).

Sizes: k = 0 (a copy), 1 (one butterfly, no multiplication), 2, 3, 6 (32 butterflies: one wavefront of the multiplying kernel,
two lanes each), 7 and 8 (two and four wavefronts; 64 and 128 butterflies are one and two wavefronts' worth of outputs per half)
with every byte of both directions compared; the inputs that make a butterfly's additions exceptional at k = 3; at k = 10 the
property the transform is for, <v, inverse(g)> = <inverse_ntt(v), g>, both sides by the oracle's MSM, and the round trip.
Outputs are pre-filled with 0xAA.  A reference is computed once per (curve, k, direction)."""
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import g1_ntt_util as GU  # noqa: E402
import ntt_util as NU  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "pallas"]
MAX_K = 8


@pytest.fixture(scope="module")
def G():
    from snark_verifier_amd import g1_ntt

    return g1_ntt


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture()
def ctx_of(gpu_ctx, pctx):
    return lambda curve: pctx if curve == "pallas" else gpu_ctx


def _dev(raw):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _filled(nbytes):
    import torch

    return torch.full((nbytes,), 0xAA, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def shared():
    """per curve 2^MAX_K random points (multiples of the generator), never changed; the references computed so far"""
    out = {"ref": {}}
    for curve in CURVES:
        O = GU.CURVES[curve]
        rnd = random.Random("gpu-g1-ntt-" + curve)
        pts, p = [], O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R))
        for _ in range(1 << MAX_K):  # a walk of random small steps: cheaper than a full multiplication per point
            pts.append(p)
            p = O.g1_add(p, O.g1_mul(O.G1_GEN, rnd.randrange(1, 1 << 32)))
        out[curve] = pts
    return out


def _reference(shared, curve, k, direction):
    key = (curve, k, direction)
    if key not in shared["ref"]:
        shared["ref"][key] = GU.pack(curve, GU.reference(curve, shared[curve][:1 << k], direction))
    return shared["ref"][key]


@pytest.mark.parametrize("k", [0, 1, 2, 3, 6, 7, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_forward_and_inverse_every_byte(G, ctx_of, shared, curve, k):
    import torch

    ctx, size = ctx_of(curve), 64 << k
    raw = GU.pack(curve, shared[curve][:1 << k])
    d_in, d_fwd, d_inv, d_back = _dev(raw), _filled(size), _filled(size), _filled(size)
    torch.cuda.synchronize()
    G.ntt_dev(ctx, d_in, d_fwd, k)
    G.intt_dev(ctx, d_in, d_inv, k)
    G.intt_dev(ctx, d_fwd, d_back, k)
    ctx.sync()
    assert _bytes(d_in) == raw  # the input is only read
    assert _bytes(d_back) == raw  # the round trip
    assert _bytes(d_fwd) == _reference(shared, curve, k, GU.FORWARD)
    assert _bytes(d_inv) == _reference(shared, curve, k, GU.INVERSE)


@pytest.mark.parametrize("curve", CURVES)
def test_exceptional_inputs(G, ctx_of, curve):
    import torch

    ctx, k = ctx_of(curve), 3
    cases = GU.special_inputs(curve, 1 << k)
    bufs = {}
    for name, pts in cases.items():
        bufs[name] = (_dev(GU.pack(curve, pts)), _filled(64 << k), _filled(64 << k))
    torch.cuda.synchronize()
    for d_in, d_fwd, d_inv in bufs.values():
        G.ntt_dev(ctx, d_in, d_fwd, k)
        G.intt_dev(ctx, d_in, d_inv, k)
    ctx.sync()
    for name, pts in cases.items():
        _, d_fwd, d_inv = bufs[name]
        assert _bytes(d_fwd) == GU.pack(curve, GU.reference(curve, pts, GU.FORWARD)), name
        assert _bytes(d_inv) == GU.pack(curve, GU.reference(curve, pts, GU.INVERSE)), name


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_in_place_equals_out_of_place_and_stays_inside_its_output(G, ctx_of, shared, curve, k):
    import torch

    ctx, size, guard = ctx_of(curve), 64 << k, 4096
    raw = GU.pack(curve, shared[curve][:1 << k])
    for fn, direction in ((G.ntt_dev, GU.FORWARD), (G.intt_dev, GU.INVERSE)):
        d_in, d_a, d_out = _dev(raw), _dev(raw), _filled(guard + size + guard)
        torch.cuda.synchronize()
        fn(ctx, d_in, d_out.data_ptr() + guard, k)
        fn(ctx, d_a, d_a, k)
        ctx.sync()
        got = _bytes(d_out)
        assert got[:guard] == b"\xaa" * guard and got[-guard:] == b"\xaa" * guard
        assert got[guard:-guard] == _bytes(d_a) == _reference(shared, curve, k, direction)


@pytest.mark.parametrize("curve", CURVES)
def test_partial_overlap_is_refused_and_nothing_is_written(G, ctx_of, shared, curve):
    import torch

    import snark_verifier_amd as sv

    ctx, k = ctx_of(curve), 3
    size = 64 << k
    raw = GU.pack(curve, shared[curve][:2 << k])
    d_buf = _dev(raw)
    torch.cuda.synchronize()
    for fn in (G.ntt_dev, G.intt_dev):
        for off in (64, size - 64):
            for i, o in ((d_buf.data_ptr(), d_buf.data_ptr() + off), (d_buf.data_ptr() + off, d_buf.data_ptr())):
                with pytest.raises(sv.SnarkvError) as e:
                    fn(ctx, i, o, k)
                assert e.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(e.value)
    with pytest.raises(sv.SnarkvError) as e:
        G.ntt_dev(ctx, d_buf, d_buf, G.max_k(ctx) + 1)
    assert e.value.code == sv.SNARKV_ERR_LENGTH
    ctx.sync()
    assert _bytes(d_buf) == raw


@pytest.mark.parametrize("curve", CURVES)
def test_committing_values_over_the_lagrange_basis_is_committing_coefficients(G, ctx_of, curve):
    """k = 10: <v, inverse(g)> = <inverse_ntt(v), g> for one random v, both sides by the oracle's Pippenger; and
    forward(inverse(g)) = g.  g is a walk of small random steps from a random point."""
    import torch

    O, ctx, k = GU.CURVES[curve], ctx_of(curve), 10
    n = 1 << k
    rnd = random.Random("gpu-g1-ntt-property-" + curve)
    g, p = [], O.g1_mul(O.G1_GEN, rnd.randrange(1, O.R))
    for _ in range(n):
        g.append(p)
        p = O.g1_add(p, O.g1_mul(O.G1_GEN, rnd.randrange(1, 1 << 24)))
    raw = GU.pack(curve, g)
    d_g, d_lag, d_back = _dev(raw), _filled(64 * n), _filled(64 * n)
    torch.cuda.synchronize()
    G.intt_dev(ctx, d_g, d_lag, k)
    G.ntt_dev(ctx, d_lag, d_back, k)
    ctx.sync()
    assert _bytes(d_back) == raw
    lagrange = GU.unpack(curve, _bytes(d_lag))
    v = [rnd.randrange(O.R) for _ in range(n)]
    coeffs = NU.reference(curve, v, NU.INVERSE)
    assert O.g1_msm_pippenger(v, lagrange) == O.g1_msm_pippenger(coeffs, g) is not None


def _key(curve, ctx, raw, k=None, first=None):
    """a resident key of the context's library: all the points, or -- with k and first -- a shard"""
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    if curve == "bn254":
        return sv.IpaDecidingKey(ctx, raw) if k is None else sv.IpaDecidingKey(ctx, raw, k=k, first=first)
    if k is None:
        return ctx.ipa_dk_create(raw)
    h = ctypes.c_void_p()
    rc = ctx._lib.snarkv_pallas_ipa_dk_create_shard(ctx._h, raw, len(raw) // 64, k, first, ctypes.byref(h))
    assert rc == 0
    return PL.PallasIpaDecidingKey(ctx._lib, h, ctx)


@pytest.mark.parametrize("curve", CURVES)
def test_the_lagrange_basis_of_a_resident_key(G, ctx_of, shared, curve):
    """dk_lagrange_dev is the inverse transform of the key's points; a shard is refused; and at k = 5 the batched commitment
    of the device's inverse_ntt(v) over the key is the Pippenger MSM of v over the key's device-made Lagrange basis"""
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_batch, ntt

    O, ctx, k = GU.CURVES[curve], ctx_of(curve), 5
    n = 1 << k
    raw = GU.pack(curve, shared[curve][:n])
    dk = _key(curve, ctx, raw)
    shard = _key(curve, ctx, raw[:64 * (n // 2)], k=k, first=n // 2)
    try:
        v = [random.Random("gpu-g1-ntt-dk-" + curve).randrange(O.R) for _ in range(n)]
        d_v, d_coeffs = _dev(NU.pack(v)), _filled(32 * n)
        d_lag, d_commit, d_msm = _filled(64 * n), _filled(64), _filled(64)
        torch.cuda.synchronize()
        G.dk_lagrange_dev(ctx, dk, d_lag)
        ntt.intt_dev(ctx, d_v, d_coeffs, k)
        ipa_batch.commit_batch_dev(ctx, dk, d_coeffs.data_ptr(), n, 1, d_commit.data_ptr())
        ctx.msm_pippenger_dev(d_v.data_ptr(), d_lag.data_ptr(), n, d_msm.data_ptr())
        with pytest.raises(sv.SnarkvError) as e:
            G.dk_lagrange_dev(ctx, shard, d_msm)
        assert e.value.code == sv.SNARKV_ERR_LENGTH and "shard" in str(e.value)
        ctx.sync()
        assert _bytes(d_lag) == _reference(shared, curve, k, GU.INVERSE)
        assert _bytes(d_commit) == _bytes(d_msm) != b"\xaa" * 64
        assert _bytes(d_commit) == O.g1_to_bytes(O.g1_msm_pippenger(NU.reference(curve, v, NU.INVERSE), shared[curve][:n]))
    finally:
        shard.close()
        dk.close()
