"""GPU: the Pippenger of the pasta build (libsnarkv_pallas.so) at the edges of its schedule, against the pallas oracle or
the expected point of a planned input (tests/msm_edge_util.py; the inputs themselves are checked on the CPU in
tests/test_msm_edge_util.py).  The kernels are the BN254 library's, compiled with pallas' p, r, GLV lattice, beta and b;
r > 2^254, so bit 254 of a canonical scalar can be set.  Covered here: the piece caps 32, 16 and 128 (the sizes at which
one MSM without the hint picks them), split buckets of the fix-up's two lists with partials that are degenerate or read
as the identity, the level-2 sort at its LDS cap, tiles, explicit window sizes, carry chains of the digit recoders,
scalar edges particular to pallas, and halo2curves' in-memory form (SNARKV_FLAG_MONTGOMERY) on every MSM entry point.
The pasta build has no C oracle and sampling a point costs about a millisecond: the points cycle through one base of
1 024, and an MSM over them is folded on the host to 1 024 terms for the oracle."""
import functools
import random

import pytest

import mont_util as M
import msm_edge_util as E
import pallas as PA

pytestmark = pytest.mark.gpu

PL = E.curve("pallas")
NB = E.PALLAS_BASE
FILL = [1000 + 7 * i for i in range(300)]


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as lib

    c = lib.PallasContext(0)
    yield c
    c.close()


def _dev(b):
    import torch

    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _run(ctx, s, p, c=0):
    import torch

    ds, dp = _dev(s), _dev(p)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.msm_pippenger_dev(ds.data_ptr(), dp.data_ptr(), len(s) // 32, out.data_ptr(), window_bits=c)
    ctx.sync()
    return bytes(out.cpu().numpy())


def _enc(scalars):
    return b"".join(PA.fe_to_bytes(x) for x in scalars)


def _cycled(n):
    """n points: the base, over and over"""
    base = PL.base_bytes(NB)
    return (base * ((n + NB - 1) // NB))[:64 * n]


@functools.lru_cache(maxsize=None)
def _random_case(seed, n):
    """n random scalars on the cycled base -> (scalar bytes, expected affine bytes)"""
    rnd = random.Random(seed)
    sc = [rnd.randrange(PA.R) for _ in range(n)]
    return _enc(sc), E.fold_to_base(PL, sc, NB)


# ---- planned buckets around each cap one MSM picks without the hint ----
def _marks(L, kind):
    """P twice / P and -P in whole buckets and in split ones, as test_duplicate_and_opposite_points of the BN254 suite"""
    return [(5, ("marks", [(1, kind)])), (L - 12, ("marks", [(L - 13, kind)])), (L + 1, ("marks", [(L, kind)])),
            (L + 8, ("marks", [(1, kind), (L + 7, kind)])), (4 * L + 1, ("marks", [(4 * L, kind)])),
            (2 * L + 1, ("marks", [(j, kind if j % 2 else "dup") for j in range(1, 2 * L + 1)]))]


def _around(L):
    """bucket lengths around the cap, and the +-P plans of both split lists: L + 2 and 2 L + 1 (lane per bucket), 24 L (at
    kBigPieces), 25 L + 1 and 25 L + 2 (past it: the cooperative list, every partial degenerate)"""
    specs = [(ln, "distinct") for ln in (L - 1, L, L + 1, 2 * L + 1)]
    for ln in (L + 2, 2 * L + 1, 24 * L, 25 * L + 1, 25 * L + 2):
        specs += E.pm_kinds(ln)
    return specs


@pytest.mark.parametrize("kind", ["dup", "neg"])
def test_planned_buckets_at_cap_32(pctx, kind):
    specs = _around(32) + _marks(32, kind) + [(24 * 32 + 1, ("marks", [(400, kind)]))]  # 25 pieces with one pair
    plan = E.plan_buckets(PL, specs, FILL)
    assert E.pip_plan(plan.n, 16)[5] == 32
    want = plan.expected()
    assert _run(pctx, plan.s, plan.p, 16) == want
    assert pctx.msm_pippenger(plan.s, plan.p) == want  # the window size of the default rule


@pytest.mark.parametrize("kind", ["dup", "neg"])
def test_planned_buckets_at_cap_16(pctx, kind):
    n = 132000
    assert E.pip_plan(n, 16)[5] == 16
    specs = _around(16) + _marks(16, kind) + [(16 * 24 + 1, "distinct"), (16 * 25 + 1, ("marks", [(200, kind)]))]
    plan = E.plan_buckets(PL, specs, E.fill_digits(n - sum(s[0] for s in specs), 1001, 30001))
    assert plan.n == n
    assert _run(pctx, plan.s, plan.p, 16) == plan.expected()


@pytest.mark.parametrize("kind", ["dup", "neg"])
def test_planned_buckets_at_cap_128(pctx, kind):
    """600 000 terms: the smallest round size at which the pasta build, which has no hint entry point, picks the cap 128"""
    n = 600000
    assert E.pip_plan(n, 16)[5] == 128 and E.pip_plan(589824, 16)[5] == 32
    specs = _around(128) + _marks(128, kind)
    plan = E.plan_buckets(PL, specs, E.fill_digits(n - sum(s[0] for s in specs), 1001, 30001))
    assert plan.n == n
    assert _run(pctx, plan.s, plan.p, 16) == plan.expected()


# ---- the level-2 sort at its LDS cap ----
@pytest.mark.parametrize("n", [7167, 7168, 7169])
def test_level2_sort_at_the_lds_cap(pctx, n):
    assert E.pip_plan(n, 16)[3] == 10
    plan = E.plan_buckets(PL, [], E.fill_digits(n, 1, 1023))
    assert _run(pctx, plan.s, plan.p, 16) == plan.expected()


def test_level2_sort_both_paths_in_one_launch(pctx):
    fill = list(E.fill_digits(7169, 1, 1023)) + list(E.fill_digits(7167, 1025, 1023))
    assert E.pip_plan(len(fill), 16)[3] == 10
    plan = E.plan_buckets(PL, [], fill)
    assert _run(pctx, plan.s, plan.p, 16) == plan.expected()


# ---- tiles, window sizes, skew, zeros ----
@pytest.mark.parametrize("n", [2047, 2048, 2049, 16379])
def test_tile_partition(pctx, n):
    s, want = _random_case(0x71, n)
    assert _run(pctx, s, _cycled(n)) == want
    if n == 16379:
        assert pctx.msm_pippenger(s, _cycled(n)) == want


@pytest.mark.parametrize("c", [2, 3, 5, 8, 11, 13, 16, 17])
def test_explicit_window_sizes(pctx, c):
    s, want = _random_case(0x72, 2000)
    assert _run(pctx, s, _cycled(2000), c) == want


def test_all_scalars_equal_and_half_equal(pctx):
    """one bucket per window holds every entry -- and every base point 16 times, so its pieces are degenerate too"""
    n = 1 << 14
    rnd = random.Random(0x73)
    k = rnd.randrange(PA.R)
    assert _run(pctx, PA.fe_to_bytes(k) * n, _cycled(n)) == E.fold_to_base(PL, [k] * n, NB)
    sc = [k] * (n // 2) + [rnd.randrange(PA.R) for _ in range(n // 2)]
    assert _run(pctx, _enc(sc), _cycled(n)) == E.fold_to_base(PL, sc, NB)


def test_zero_scalars_and_empty_buckets(pctx):
    n = 600
    rnd = random.Random(0x74)
    sc = [0 if i % 3 == 0 else rnd.randrange(PA.R) for i in range(n)]
    assert _run(pctx, _enc(sc), _cycled(n), 17) == E.fold_to_base(PL, sc, NB)  # 2^16 buckets per window, almost all empty
    assert _run(pctx, bytes(32 * n), _cycled(n)) == bytes(64)
    assert pctx.msm_pippenger(bytes(32 * n), _cycled(n)) == bytes(64)


# ---- carry chains of the digit recoders ----
@functools.lru_cache(maxsize=None)
def _crafted():
    return tuple(k for c in (13, 16) for k, _, _ in E.crafted_scalars(PL, c))


@functools.lru_cache(maxsize=None)
def _crafted_case():
    ks = _crafted()
    n = 2000 + len(ks)
    rnd = random.Random(0x75)
    sc = [rnd.randrange(PA.R) for _ in range(n)]
    for i, k in enumerate(ks):
        sc[7 + i * (n // len(ks))] = k
    return _enc(sc), E.fold_to_base(PL, sc, NB), n


@pytest.mark.parametrize("c", [13, 16])
def test_carry_chains_among_random_terms(pctx, c):
    assert 150 <= len(_crafted()) <= 300
    s, want, n = _crafted_case()
    assert _run(pctx, s, _cycled(n), c) == want


@functools.lru_cache(maxsize=None)
def _crafted_alone():
    base = PL.base_bytes(NB)
    return tuple(PL.mul(base[64 * i:64 * i + 64], k) for i, k in enumerate(_crafted()))


@pytest.mark.parametrize("c", [13, 16])
def test_carry_chains_one_term_each(pctx, c):
    import torch

    ks, want = _crafted(), _crafted_alone()
    ds, dp = _dev(_enc(ks)), _dev(PL.base_bytes(NB))
    out = torch.zeros(len(ks), 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(len(ks)):
        pctx.msm_pippenger_dev(ds.data_ptr() + 32 * i, dp.data_ptr() + 64 * i, 1, out[i].data_ptr(), window_bits=c)
    pctx.sync()
    got = bytes(out.cpu().numpy())
    for i, k in enumerate(ks):
        assert got[64 * i:64 * i + 64] == want[i], (i, hex(k))


# ---- scalar edges particular to pallas ----
def _edge_scalars():
    R, lam = PA.R, PL.lam
    return [1 << 254, (1 << 254) + 1, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, lam, R - lam, (lam + 1) % R, lam * lam % R,
            (1 << 127) - 1, (1 << 127) + 1, 1 << 128]


def test_scalar_edges_alone_and_together(pctx):
    """r > 2^254: bit 254 of a canonical scalar can be set (never on BN254); lambda and its neighbours put one GLV half at
    0 or 1; 2^127 +- 1 and 2^128 sit where the halves change their shape"""
    ks = _edge_scalars()
    assert all(0 < k < PA.R for k in ks) and ks[0] >> 254 == 1
    base = PL.base_bytes(NB)
    for i, k in enumerate(ks):
        q = base[64 * i:64 * i + 64]
        want = PL.mul(q, k)
        assert pctx.msm_pippenger(PA.fe_to_bytes(k), q) == want, hex(k)
        assert _run(pctx, PA.fe_to_bytes(k), q, 16) == want, hex(k)
    want = PL.msm(ks, base[:64 * len(ks)])
    for c in (0, 13, 16):
        assert _run(pctx, _enc(ks), base[:64 * len(ks)], c) == want, c
    assert pctx.msm_pippenger(_enc(ks), base[:64 * len(ks)]) == want


# ---- halo2curves' in-memory form on the MSM entry points (snarkv_pallas_ctx_set_flags) ----
def _s_mont(s):
    return b"".join(M.fe_to_mont(s[i:i + 32], PA.R) for i in range(0, len(s), 32))


def _p_mont(p):
    return b"".join(M.fe_to_mont(p[i:i + 32], PA.P) for i in range(0, len(p), 32))


@pytest.fixture()
def mctx():
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as lib

    c = lib.PallasContext(0)
    c.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
    yield c
    c.close()


def _mont_case(n=300, identity=True):
    """scalars with the edges among them, points with the identity, P twice and P, -P among them"""
    rnd = random.Random(0x76)
    sc = (_edge_scalars() + [0, 1] + [rnd.randrange(PA.R) for _ in range(n)])[:n]
    base = PL.base_bytes(NB)
    p = bytearray(base[:64 * n])
    if identity:
        p[64 * 20:64 * 21] = bytes(64)                # the identity: 64 zero bytes in both forms
    p[64 * 22:64 * 23] = p[64 * 21:64 * 22]           # P twice
    p[64 * 24:64 * 25] = PA.g1_to_bytes(PA.g1_neg(PA.g1_from_bytes(bytes(p[64 * 23:64 * 24]))))
    s, p = _enc(sc), bytes(p)
    return sc, s, p, PL.msm(sc, p)  # (the oracle takes the identity as a point like any other)


def test_in_memory_form_on_every_msm_entry_point(mctx):
    import snark_verifier_amd as sv

    sc, s, p, want = _mont_case()
    sm, pm = _s_mont(s), _p_mont(p)
    assert pm[64 * 20:64 * 21] == bytes(64) and sm != s and _p_mont(want) != want
    assert mctx.msm_pippenger(sm, pm) == _p_mont(want)
    assert _run(mctx, sm, pm) == _p_mont(want)
    assert _run(mctx, sm, pm, 16) == _p_mont(want)
    offs = [0, 5, 17, 64]
    segs = [PL.msm(sc[a:b], p[64 * a:64 * b]) for a, b in zip(offs, offs[1:])]
    assert mctx.msm_batched(sm[:32 * 64], pm[:64 * 64], offs) == b"".join(_p_mont(x) for x in segs)
    assert mctx.msm_naive(sm[:32 * 17], pm[:64 * 17]) == _p_mont(PL.msm(sc[:17], p[:64 * 17]))
    # the identity stays 64 zero bytes: as a result (k P - k P) ...
    q = p[64 * 23:64 * 25]
    two = _s_mont(PA.fe_to_bytes(7) * 2)
    assert mctx.msm_pippenger(two, _p_mont(q)) == bytes(64)
    assert _run(mctx, two, _p_mont(q)) == bytes(64)
    assert mctx.msm_naive(two, _p_mont(q)) == bytes(64)
    assert mctx.msm_batched(two + sm[:32], _p_mont(q) + pm[:64], [0, 2, 3])[:64] == bytes(64)
    # ... and as an input (term 20 above, and alone)
    assert mctx.msm_naive(sm[:32], bytes(64)) == bytes(64)
    # the per-call flag stays ignored on the pasta entry points: nothing changes with it set as well
    assert mctx.msm_batched(sm[:32 * 64], pm[:64 * 64], offs, flags=sv.SNARKV_FLAG_MONTGOMERY) == b"".join(_p_mont(x) for x in segs)
    # clearing the flag restores the wire form, on the same context
    mctx.set_flags(0)
    assert mctx.msm_pippenger(s, p) == want
    assert _run(mctx, s, p) == want
    assert mctx.msm_batched(s[:32 * 64], p[:64 * 64], offs) == b"".join(segs)
    assert mctx.msm_batched(s[:32 * 64], p[:64 * 64], offs, flags=sv.SNARKV_FLAG_MONTGOMERY) == b"".join(segs)
    assert mctx.msm_naive(s[:32 * 17], p[:64 * 17]) == PL.msm(sc[:17], p[:64 * 17])


def test_decompress_then_msm_without_re_encoding(mctx):
    """the product flow on a context that speaks the in-memory form: `g1_decompress` of wire-form encodings leaves
    in-memory points, and the MSM takes them as they are"""
    n = 200
    rnd = random.Random(0x77)
    sc = [rnd.randrange(PA.R) for _ in range(n)]
    base = PL.base_bytes(NB)[:64 * n]
    comp = bytearray()
    for i in range(n):
        x, y = PA.g1_from_bytes(base[64 * i:64 * i + 64])
        comp += (x | ((y & 1) << 255)).to_bytes(32, "little")
    pts, ok = mctx.g1_decompress(bytes(comp))
    assert all(ok) and pts == _p_mont(base)
    assert _run(mctx, _s_mont(_enc(sc)), pts) == _p_mont(PL.msm(sc, base))


def test_validate_together_with_the_in_memory_default():
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as lib

    sc, s, p, want = _mont_case(64, identity=False)
    sm, pm = _s_mont(s), _p_mont(p)
    ctx = lib.PallasContext(0)
    try:
        ctx.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
        # the validate flag per call, the in-memory form from the context
        assert ctx.msm_naive(sm, pm, flags=sv.SNARKV_FLAG_VALIDATE) == _p_mont(want)
        assert ctx.msm_batched(sm, pm, [0, 30, 64], flags=sv.SNARKV_FLAG_VALIDATE)[:64] == _p_mont(PL.msm(sc[:30], p[:64 * 30]))
        off_curve = _p_mont(PA.fe_to_bytes(5) + PA.fe_to_bytes(7))
        with pytest.raises(sv.SnarkvError):
            ctx.msm_naive(sm[:32], off_curve, flags=sv.SNARKV_FLAG_VALIDATE)
        # a point that is on the curve in the wire form is not in the in-memory form
        with pytest.raises(sv.SnarkvError):
            ctx.msm_naive(sm[:32], p[:64], flags=sv.SNARKV_FLAG_VALIDATE)
        # both as defaults of the context: every entry point validates
        ctx.set_flags(sv.SNARKV_FLAG_MONTGOMERY | sv.SNARKV_FLAG_VALIDATE)
        assert ctx.msm_pippenger(sm, pm) == _p_mont(want)
        assert ctx.msm_naive(sm, pm) == _p_mont(want)
        with pytest.raises(sv.SnarkvError):
            ctx.msm_pippenger(sm[:64], pm[:64] + off_curve)
        with pytest.raises(sv.SnarkvError):
            ctx.msm_batched(sm[:64], pm[:64] + off_curve, [0, 2])
        assert ctx.msm_pippenger(sm, pm) == _p_mont(want)  # the context goes on working after a refusal
    finally:
        ctx.close()
