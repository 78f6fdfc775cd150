"""GPU: the transform calls (snark_verifier_amd.ntt, include/snarkv_ntt.h) on BN254 and pallas against the reference of
tests/ntt_util.py (an iterative radix-2 transform over Python integers with the oracle's root of unity).

Sizes, with T = ntt.TILE_BITS = 9: k = 0, 1, 2, T - 1, T, T + 1, 2T - 1, 2T, 2T + 1, and 14 | 15, the sizes on both sides of the
step from two passes to three in this plan (a pass of several takes at most T - 2 = 7 levels: one pass up to k = 9, two up to
14, three up to 21; the first four-pass size, 2^22, is above the 2^20 this file stops at and is covered by the host model,
tests/test_ntt_model.py, whose tiles of 2^1 .. 2^3 take up to ten passes).  Up to k = 17 every byte of the forward and of the
inverse transform is compared; above, the dense round trip, four outputs by Horner and a sparse input in full.  Outputs are
pre-filled with 0xAA; every case synchronises once."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ntt_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
T = 9
SIZES = [0, 1, 2, T - 1, T, T + 1, 14, 15, 2 * T - 1, 2 * T, 2 * T + 1]
MAX_K = max(SIZES)
DENSE_UP_TO = 17
assert MAX_K <= 20


@pytest.fixture(scope="module")
def N():
    from snark_verifier_amd import ntt

    assert ntt.TILE_BITS == T
    return ntt


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
    """per curve: 2^MAX_K random elements, as integers, packed and on the device -- computed once, never changed; and the
    references computed so far, (curve, k, direction) -> values"""
    import torch

    out = {"ref": {}}
    for curve, cv in U.CURVES.items():
        rnd = random.Random("gpu-ntt-" + curve)
        vals = [rnd.randrange(cv.R) for _ in range(1 << MAX_K)]
        raw = U.pack(vals)
        out[curve] = (vals, raw, _dev(raw))
    torch.cuda.synchronize()
    return out


def _reference(shared, curve, k, direction):
    key = (curve, k, direction)
    if key not in shared["ref"]:
        shared["ref"][key] = U.pack(U.reference(curve, shared[curve][0][:1 << k], direction))
    return shared["ref"][key]


def _sparse_indices(k):
    """8 places: 0, 1, n - 1 and both sides of a tile boundary (2^T) and of the half (the top digit's step)"""
    n = 1 << k
    return [0, 1, (1 << T) - 1, 1 << T, (1 << T) + 1, n // 2 - 1, n // 2, n - 1]


def _sparse_forward(curve, k, terms):
    """the transform of sum_m c_m X^(j_m) in full: out[i] = sum_m c_m (w^(j_m))^i by running products"""
    r = U.CURVES[curve].R
    w = U.omega(curve, k)
    steps = [pow(w, j, r) for j, _ in terms]
    cur = [c for _, c in terms]
    out = []
    for _ in range(1 << k):
        out.append(sum(cur) % r)
        cur = [c * s % r for c, s in zip(cur, steps)]
    return out


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_forward_and_inverse(N, ctx_of, shared, curve, k):
    import torch

    r, ctx, n = U.CURVES[curve].R, ctx_of(curve), 1 << k
    vals, raw, d_in = shared[curve]
    size = 32 * n
    d_fwd, d_inv, d_back, d_sparse_out = _filled(size), _filled(size), _filled(size), _filled(size)
    dense = k <= DENSE_UP_TO
    if not dense:
        rnd = random.Random("gpu-ntt-sparse-%s-%d" % (curve, k))
        terms = [(j, rnd.randrange(1, r)) for j in _sparse_indices(k)]
        sparse = [0] * n
        for j, c in terms:
            sparse[j] = c
        d_sparse = _dev(U.pack(sparse))
    torch.cuda.synchronize()
    N.ntt_dev(ctx, d_in, d_fwd, k)
    N.intt_dev(ctx, d_in, d_inv, k)
    N.intt_dev(ctx, d_fwd, d_back, k)
    if not dense:
        N.ntt_dev(ctx, d_sparse, d_sparse_out, k)
    ctx.sync()
    fwd, inv = _bytes(d_fwd), _bytes(d_inv)
    assert _bytes(d_back) == raw[:size]  # the dense round trip, every byte
    assert _bytes(d_in[:size]) == raw[:size]  # the input is only read
    if dense:
        assert fwd == _reference(shared, curve, k, U.FORWARD)
        assert inv == _reference(shared, curve, k, U.INVERSE)
        return
    w, got = U.omega(curve, k), U.unpack(fwd)
    for i in (0, 1, n // 2, n - 1):
        assert got[i] == U.horner(vals[:n], pow(w, i, r), r), i
    assert inv != fwd and inv != b"\xaa" * size  # (the inverse itself is held by the round trip above)
    assert _bytes(d_sparse_out) == U.pack(_sparse_forward(curve, k, terms))


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_shift_is_the_coset(N, ctx_of, shared, curve):
    import torch

    r, ctx, k = U.CURVES[curve].R, ctx_of(curve), T + 1
    n = 1 << k
    vals, raw, d_in = shared[curve]
    s = random.Random("gpu-ntt-shift-" + curve).randrange(2, r)
    d_coset, d_back, d_inv = _filled(32 * n), _filled(32 * n), _filled(32 * n)
    torch.cuda.synchronize()
    N.ntt_dev(ctx, d_in, d_coset, k, shift=s)
    N.intt_dev(ctx, d_coset, d_back, k, shift=pow(s, -1, r))
    N.intt_dev(ctx, d_in, d_inv, k, shift=s)
    ctx.sync()
    w, got = U.omega(curve, k), U.unpack(_bytes(d_coset))
    for i in [0, 1, 2, 3, 127, 128, 129, 511, 512, 513, n // 2 - 1, n // 2, n // 2 + 1, n - 3, n - 2, n - 1]:
        assert got[i] == U.horner(vals[:n], s * pow(w, i, r) % r, r), i
    assert _bytes(d_back) == raw[:32 * n]  # the inverse with s^-1 restores the input
    assert _bytes(d_inv) == U.pack(U.reference(curve, vals[:n], U.INVERSE, s))  # ... and with s it is the header's sum, in full


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_batch_equals_single_calls_and_stays_inside_its_output(N, ctx_of, shared, curve):
    import torch

    ctx, k, count, guard = ctx_of(curve), T + 1, 3, 4096
    size = 32 << k
    _, _, d_in = shared[curve]
    for fn in (N.ntt_dev, N.intt_dev):
        d_batch = _filled(guard + count * size + guard)
        d_single = _filled(count * size)
        torch.cuda.synchronize()
        fn(ctx, d_in, d_batch.data_ptr() + guard, k, count=count)
        for j in range(count):
            fn(ctx, d_in.data_ptr() + j * size, d_single.data_ptr() + j * size, k)
        ctx.sync()
        got = _bytes(d_batch)
        assert got[:guard] == b"\xaa" * guard and got[-guard:] == b"\xaa" * guard
        assert got[guard:-guard] == _bytes(d_single)
        assert len(set(got[guard + j * size:guard + (j + 1) * size] for j in range(count))) == count  # three different polynomials


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_tables_are_refilled_when_the_scratch_grows(N, shared, curve):
    """a fresh context: the second call has the same (k, direction) as the first and a larger batch, so the slot that holds the
    tables of powers is allocated anew between them"""
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    k, count = T + 1, 5
    size = 32 << k
    _, _, d_in = shared[curve]
    ctx = PL.PallasContext(0) if curve == "pallas" else sv.Context(0)
    try:
        d_one, d_many = _filled(size), _filled(count * size)
        torch.cuda.synchronize()
        N.ntt_dev(ctx, d_in, d_one, k)
        N.ntt_dev(ctx, d_in, d_many, k, count=count)
        ctx.sync()
        assert _bytes(d_one) == _reference(shared, curve, k, U.FORWARD) == _bytes(d_many[:size])
        d_back = _filled(count * size)
        N.intt_dev(ctx, d_many, d_back, k, count=count)
        ctx.sync()
        assert _bytes(d_back) == shared[curve][1][:count * size]
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [2, T, T + 1, 15])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_in_place_equals_out_of_place(N, ctx_of, shared, curve, k):
    import torch

    r, ctx, count = U.CURVES[curve].R, ctx_of(curve), 2
    size = count * 32 << k
    _, raw, d_in = shared[curve]
    s = random.Random("gpu-ntt-inplace").randrange(2, r)
    for fn in (N.ntt_dev, N.intt_dev):
        d_a, d_b, d_out = _dev(raw[:size]), _dev(raw[:size]), _filled(2 * size)
        torch.cuda.synchronize()
        fn(ctx, d_in, d_out, k, count=count)
        fn(ctx, d_in, d_out.data_ptr() + size, k, count=count, shift=s)
        fn(ctx, d_a, d_a, k, count=count)
        fn(ctx, d_b, d_b, k, count=count, shift=s)
        ctx.sync()
        assert _bytes(d_a) + _bytes(d_b) == _bytes(d_out)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_partial_overlap_is_refused_and_nothing_is_written(N, ctx_of, shared, curve):
    import torch

    import snark_verifier_amd as sv

    ctx, k = ctx_of(curve), T + 1
    size = 32 << k
    _, raw, _ = shared[curve]
    d_buf = _dev(raw[:2 * size])
    torch.cuda.synchronize()
    for fn in (N.ntt_dev, N.intt_dev):
        for off in (32, size - 32, size // 2):
            with pytest.raises(sv.SnarkvError) as e:
                fn(ctx, d_buf, d_buf.data_ptr() + off, k)
            assert e.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(e.value)
            with pytest.raises(sv.SnarkvError) as e:
                fn(ctx, d_buf.data_ptr() + off, d_buf, k)
            assert e.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(e.value)
    ctx.sync()
    assert _bytes(d_buf) == raw[:2 * size]
    d_out = _filled(size)  # the context stays usable
    N.ntt_dev(ctx, d_buf, d_out, k)
    ctx.sync()
    assert _bytes(d_out) == _reference(shared, curve, k, U.FORWARD)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_worst_values(N, ctx_of, curve):
    """every input r - 1 at k = min(2T, 17): the lazy sums of every level meet the same, largest residue.  The transform of a
    constant c is n c at index 0 and zero elsewhere; the inverse one is c at index 0"""
    import torch

    r, ctx, k = U.CURVES[curve].R, ctx_of(curve), min(2 * T, 17)
    n = 1 << k
    d_in = _dev(U.pack([r - 1]) * n)
    d_fwd, d_inv = _filled(32 * n), _filled(32 * n)
    torch.cuda.synchronize()
    N.ntt_dev(ctx, d_in, d_fwd, k)
    N.intt_dev(ctx, d_in, d_inv, k)
    ctx.sync()
    zeros = bytes(32 * (n - 1))
    assert _bytes(d_fwd) == U.pack([n * (r - 1) % r]) + zeros
    assert _bytes(d_inv) == U.pack([r - 1]) + zeros


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_lagrange_values_in_opening_out(N, gpu_ctx, pctx, curve):
    """The composition the transform is for.  At k = 5 five of the six committed polynomials of the multi-open case exist on
    the device only as their evaluations over the domain; `intt_dev` turns them into coefficients in the buffer that
    `ipa_multiopen.create_proof_dev` then reads, and the proof is the oracle's `bgh19_create_proof` over the Python-side
    coefficients, byte for byte."""
    import torch

    import ipa as I
    import kzg as K
    from snark_verifier_amd import ipa_multiopen as MO
    from test_gpu_ipa_multiopen import Case

    mod = U.CURVES[curve]
    ctx = pctx if curve == "pallas" else gpu_ctx
    I.use_curve(mod)
    K.use_curve(mod)
    try:
        k, lagrange = 5, 5
        c = Case(ctx, curve, k, "lagrange")
        columns = [U.reference(curve, p, U.FORWARD) for p in c.polys[:lagrange]]  # what a prover holds
        I.use_curve(mod)  # (the reference switches the oracle for its root of unity and back)
        K.use_curve(mod)
        d_polys = _dev(b"".join(U.pack(v) for v in columns + c.polys[lagrange:]))
        d_bar = _dev(U.pack(c.p_bar))
        torch.cuda.synchronize()
        N.intt_dev(ctx, d_polys, d_polys, k, count=lagrange)  # in place, on the context's stream, before the prover's kernels
        proof, acc = MO.create_proof_dev(ctx, c.dk, c.pk.h, c.pk.s, d_polys.data_ptr(), len(c.polys), c.blinds, c.x, c.queries,
                                         c.f_blind, d_bar.data_ptr(), c.omega_bar)
        assert proof == c.oracle()
        assert _bytes(d_polys) == b"".join(U.pack(p) for p in c.polys)
        c.close()
    finally:
        I.use_curve(U.BN)
        K.use_curve(U.BN)
