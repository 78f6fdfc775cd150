"""GPU: the resident-polynomial calls (snark_verifier_amd.poly, include/snarkv_poly.h) on BN254 and pallas against Python
integers: division by a linear factor and evaluation at lengths on both sides of one block of the scan (256 coefficients)
and of one block of blocks (256^2 = 65 536), the exact multiple and the off-by-one, the header's no-overlap promise, and the
linear combination with term counts on both sides of its lazy-sum bound (4 terms) and of one pass (32 terms)."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as O  # noqa: E402
import pallas as PA  # noqa: E402

pytestmark = pytest.mark.gpu
FIELD = {"bn254": O.R, "pallas": PA.R}
# 256 = the scan's block (poly.BLOCK): 255 | 256 | 257 around one block, 65 535 | 65 536 | 65 537 around one block of blocks,
# 2^17 + 3 = three levels with a ragged last block on each
LENGTHS = [1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 17) + 3]
MAX_N = max(LENGTHS)


@pytest.fixture(scope="module")
def P():
    from snark_verifier_amd import poly

    assert poly.BLOCK == 256 and poly.LINCOMB_TERMS == 32 and poly.LAZY_TERMS == 4
    return poly


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture()
def ctx_of(gpu_ctx, pctx):
    return lambda curve: pctx if curve == "pallas" else gpu_ctx


def _pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _dev(raw):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _ints(t):
    raw = t.cpu().numpy().tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.fixture(scope="module")
def shared():
    """per curve: MAX_N random coefficients, as integers and on the device -- computed once, never changed"""
    import torch

    out = {}
    for curve, r in FIELD.items():
        rnd = random.Random("gpu-poly-" + curve)
        p = [rnd.randrange(r) for _ in range(MAX_N)]
        out[curve] = (p, _dev(_pack(p)), rnd.randrange(2, r))
    torch.cuda.synchronize()
    return out


def div_linear(p, a, r):
    """oracle/ipa.py::_poly_div_linear with the remainder kept"""
    out, carry = [0] * (len(p) - 1), 0
    for i in range(len(p) - 1, 0, -1):
        carry = (p[i] + carry * a) % r
        out[i - 1] = carry
    return out, (p[0] + carry * a) % r


def _divide(P, ctx, d_p, n, roots):
    """division and evaluation for every root, enqueued back to back, one synchronisation -> [(quot bytes, rem, value)]"""
    import torch

    d_roots = _dev(_pack(roots))
    d_quot = torch.full((len(roots), 32 * max(n - 1, 1)), 0xAA, dtype=torch.uint8, device="cuda")
    d_small = torch.full((len(roots), 2, 32), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for j in range(len(roots)):
        root = d_roots.data_ptr() + 32 * j
        P.div_linear_dev(ctx, d_p, n, root, d_quot[j].data_ptr() if n > 1 else None, d_small[j, 0].data_ptr())
        P.eval_dev(ctx, d_p, n, root, d_small[j, 1].data_ptr())
    ctx.sync()
    small = _ints(d_small)
    return [(d_quot[j].cpu().numpy().tobytes(), small[2 * j], small[2 * j + 1]) for j in range(len(roots))]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_division_and_evaluation(P, ctx_of, shared, curve, n):
    r, ctx = FIELD[curve], ctx_of(curve)
    p, d_p, rand_root = shared[curve]
    roots = [0, 1, r - 1, rand_root]
    for a, (quot, rem, val) in zip(roots, _divide(P, ctx, d_p, n, roots)):
        want_q, want_r = div_linear(p[:n], a, r)
        assert rem == want_r == val, (n, a)
        if n > 1:
            assert quot == _pack(want_q), (n, a)
        else:
            assert quot == b"\xaa" * 32  # an empty quotient: nothing is written


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_exact_multiple_and_off_by_one(P, ctx_of, shared, curve):
    import torch

    r, ctx = FIELD[curve], ctx_of(curve)
    base, _, a = shared[curve]
    n = 65537
    q = base[:n - 1]
    p = [(x - a * y) % r for x, y in zip([0] + q, q + [0])]  # (X - a) q
    d_p = _dev(_pack(p))
    torch.cuda.synchronize()
    (quot, rem, val), = _divide(P, ctx, d_p, n, [a])
    assert (rem, val) == (0, 0) and quot == _pack(q)
    p[0] = (p[0] + 1) % r
    d_p = _dev(_pack(p))
    torch.cuda.synchronize()
    (quot, rem, val), = _divide(P, ctx, d_p, n, [a])
    assert (rem, val) == (1, 1) and quot == _pack(q)


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_overlap_is_refused_and_nothing_is_written(P, ctx_of, shared, curve):
    """the header's promise: quot may not overlap coeffs (nor rem either): SNARKV_ERR_ARG, and the buffers stay as they were"""
    import torch

    import snark_verifier_amd as sv

    r, ctx = FIELD[curve], ctx_of(curve)
    p, _, a = shared[curve]
    n = 600
    d_p = _dev(_pack(p[:n]))
    d_root = _dev(_pack([a]))
    d_rem = torch.full((32,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for quot in (d_p.data_ptr(), d_p.data_ptr() + 32, d_p.data_ptr() + 32 * (n - 1)):
        with pytest.raises(sv.SnarkvError) as e:
            P.div_linear_dev(ctx, d_p, n, d_root, quot, d_rem)
        assert e.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(e.value)
    with pytest.raises(sv.SnarkvError) as e:
        P.div_linear_dev(ctx, d_p, n, d_root, d_rem, d_p.data_ptr() + 64)
    assert e.value.code == sv.SNARKV_ERR_ARG
    ctx.sync()
    assert _ints(d_p) == p[:n] and d_rem.cpu().numpy().tobytes() == b"\xaa" * 32
    (quot, rem, val), = _divide(P, ctx, d_p, n, [a])  # the context stays usable
    want_q, want_r = div_linear(p[:n], a, r)
    assert quot == _pack(want_q) and rem == val == want_r


@pytest.mark.parametrize("count", [1, 2, 4, 5, 17, 32, 33, 40])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_linear_combination(P, ctx_of, shared, curve, count):
    """count = 4 | 5 on both sides of the lazy sum's reduction, 32 | 33 of one pass, 40 = a second pass that itself reduces;
    repeated indices, the scalars 0 and r - 1 and coefficients r - 1 (the largest terms) included"""
    import torch

    import snark_verifier_amd as sv

    r, ctx = FIELD[curve], ctx_of(curve)
    base, d_base, _ = shared[curve]
    rnd = random.Random("lincomb-%s-%d" % (curve, count))
    for n in (1, 257, 1 << 16):
        n_polys = 2  # slices of the shared coefficients, poly-major, plus the all-(r - 1) polynomial for n = 257
        polys = [base[:n], base[n:2 * n]]
        d_polys = d_base
        if n == 257:
            polys.append([r - 1] * n)
            n_polys = 3
            d_polys = _dev(_pack(polys[0] + polys[1] + polys[2]))
        idx = [rnd.randrange(n_polys) for _ in range(count)]
        scalars = [rnd.choice([0, r - 1, rnd.randrange(r), rnd.randrange(r)]) for _ in range(count)]
        if n == 257:
            idx, scalars = [2] * count, [r - 1] * count  # every term (r - 1)^2: the largest the lazy sum meets
        d_out = torch.full((32 * n,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        P.lincomb_dev(ctx, d_polys, n, n_polys, idx, scalars, d_out)
        ctx.sync()
        per_poly = [sum(s for i, s in zip(idx, scalars) if i == j) % r for j in range(n_polys)]
        want = [sum(w * pl[i] for w, pl in zip(per_poly, polys)) % r for i in range(n)]
        assert d_out.cpu().numpy().tobytes() == _pack(want), (n, count)
    with pytest.raises(sv.SnarkvError) as e:  # an index past the array, on a real context: refused before any launch
        P.lincomb_dev(ctx, d_base, 4, 2, [0, 2], [1, 1], d_out)
    assert e.value.code == sv.SNARKV_ERR_ARG
