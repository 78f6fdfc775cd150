"""GPU: the Pippenger with its fast bucket additions on the friendly-multiple products (csrc/fq29.h `_fm`, selected by
SNARKV_FQ29_FM in csrc/msm_pippenger.hip) gives the oracle's bytes.  The products leave other representatives of the same
residues than the pinned ones, so what is compared is the canonical affine result.  Small sizes on purpose (1, 2, one
wavefront of entries less one / exactly / plus one, 4 097), each with the forced windows c = 4 and c = 8 -- few buckets,
hence long ones and many trips per k_accumulate lane, split buckets and the stitch of k_fixup -- and with the default
window; four scalar sets (uniform; all equal; a point, its copy and its negation in one bucket, which takes the careful
redo; the scalars 0, 1, r - 1); both encodings.  The same smallest cases through the pasta library (whose build leaves the
switch off -- the friendly multiple costs a multiply-add per step there -- so they hold the shared adder template on the
pinned products), and one many-MSM call of three ragged jobs."""
import functools
import random

import pytest

import bn254 as O
import coracle as C
import mont_util as MU
import msm_edge_util as E
import pallas as PA

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 4097]
WINDOWS = [4, 8, 0]
SETS = ["uniform", "equal", "dup_neg", "edges"]


def _dev(b):
    import torch

    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _run(ctx, s, p, c):
    import torch

    ds, dp = _dev(s), _dev(p)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.msm_pippenger_dev(ds.data_ptr(), dp.data_ptr(), len(s) // 32, out.data_ptr(), window_bits=c)
    ctx.sync()
    return bytes(out.cpu().numpy())


def _scalars(kind, n, r, seed):
    """n integer scalars of one set"""
    rnd = random.Random(seed)
    if kind == "uniform":
        return [rnd.randrange(r) for _ in range(n)]
    if kind == "equal":
        return [rnd.randrange(r)] * n
    if kind == "edges":
        return [(0, 1, r - 1)[i % 3] for i in range(n)]
    sc = [rnd.randrange(r) for _ in range(n)]  # dup_neg: terms 0, 1, 2 share a scalar (one bucket in every window)
    for i in range(1, min(n, 3)):
        sc[i] = sc[0]
    return sc


def _points(kind, pts, neg):
    """dup_neg: term 1 is a copy of term 0, term 2 its negation (`neg`: 64 bytes -> 64 bytes)"""
    if kind != "dup_neg":
        return pts
    p = bytearray(pts)
    if len(p) >= 128:
        p[64:128] = p[:64]
    if len(p) >= 192:
        p[128:192] = neg(bytes(p[:64]))
    return bytes(p)


@functools.lru_cache(maxsize=None)
def _bn_case(kind, n):
    sc = _scalars(kind, n, O.R, 0xF300 + n)
    s = b"".join(O.fe_to_bytes(x) for x in sc)
    p = _points(kind, C.sample_points(0xF400 + n, n), lambda q: O.g1_to_bytes(O.g1_neg(O.g1_from_bytes(q))))
    return s, p, C.msm_pippenger(s, p, 4)


@pytest.fixture(scope="module")
def mont_ctx():
    import snark_verifier_amd as sv

    c = sv.Context(0)
    c.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
    yield c
    c.close()


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_bn254_bytes_equal_the_oracle(gpu_ctx, mont_ctx, n, c):
    for kind in SETS:
        s, p, want = _bn_case(kind, n)
        assert _run(gpu_ctx, s, p, c) == want, (kind, "canonical")
        assert _run(mont_ctx, MU.scalars_to_mont(s), MU.coords_to_mont(p), c) == MU.coords_to_mont(want), (kind, "montgomery")


def test_many_msm_call_of_three_ragged_jobs(gpu_ctx):
    import torch

    jobs = [_bn_case("uniform", 4097), _bn_case("equal", 65), _bn_case("dup_neg", 63)]
    ds, dp = [_dev(j[0]) for j in jobs], [_dev(j[1]) for j in jobs]
    out = torch.zeros(64 * len(jobs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.msm_pippenger_many_dev([t.data_ptr() for t in ds], [t.data_ptr() for t in dp], [len(j[0]) // 32 for j in jobs],
                                   out.data_ptr())
    gpu_ctx.sync()
    got = bytes(out.cpu().numpy())
    for i, j in enumerate(jobs):
        assert got[64 * i:64 * i + 64] == j[2], i


# ---- the pasta library: the same smallest cases (its oracle is Python: the sizes up to 65)
PL = E.curve("pallas")


@functools.lru_cache(maxsize=None)
def _pallas_case(kind, n):
    sc = _scalars(kind, n, PA.R, 0xF500 + n)
    p = _points(kind, PL.base_bytes(E.PALLAS_BASE)[:64 * n], lambda q: PA.g1_to_bytes(PA.g1_neg(PA.g1_from_bytes(q))))
    return b"".join(PA.fe_to_bytes(x) for x in sc), p, PL.msm(sc, p)


@pytest.fixture(scope="module")
def pallas_ctxs():
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as lib

    a, b = lib.PallasContext(0), lib.PallasContext(0)
    b.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
    yield a, b
    a.close()
    b.close()


def _pallas_mont(b, mod):
    return b"".join(MU.fe_to_mont(b[i:i + 32], mod) for i in range(0, len(b), 32))


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_pallas_bytes_equal_the_oracle(pallas_ctxs, n, c):
    plain, mont = pallas_ctxs
    for kind in SETS:
        s, p, want = _pallas_case(kind, n)
        assert _run(plain, s, p, c) == want, (kind, "canonical")
        assert _run(mont, _pallas_mont(s, PA.R), _pallas_mont(p, PA.P), c) == _pallas_mont(want, PA.P), (kind, "montgomery")
