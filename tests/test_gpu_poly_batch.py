"""GPU: the batched evaluation (snark_verifier_amd.poly_batch, include/snarkv_poly_batch.h) on BN254 and pallas: every result
against Horner in Python integers and, byte for byte, against `poly_eval_dev` on the same polynomial and point.  Lengths: one
block of the scan (1, 255, 256), two levels (257), three levels (65 537: its 257 totals make two blocks one level up).  Counts
1, 2 and 40 with repeated polynomial and point indices, a point equal to 0 and a point equal to 1.  The bytes around the
results keep their pattern."""
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
LENGTHS = [1, 255, 256, 257, 65537]
COUNTS = [1, 2, 40]
N_POLYS, N_POINTS = 3, 5


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


def _pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _dev(raw):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def horner(p, x, r):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % r
    return acc


@pytest.fixture(scope="module")
def shared():
    """per curve and length: the polynomials and the points as integers and on the device, and every value
    polys[i](points[j]) -- computed once, never changed"""
    import torch

    out = {}
    for curve, r in FIELD.items():
        rnd = random.Random("gpu-poly-batch-" + curve)
        points = [0, 1, r - 1, rnd.randrange(2, r), rnd.randrange(2, r)]
        d_points = _dev(_pack(points))
        for n in LENGTHS:
            polys = [[rnd.randrange(r) for _ in range(n)] for _ in range(N_POLYS)]
            values = [[horner(p, x, r) for x in points] for p in polys]
            out[curve, n] = (values, _dev(b"".join(_pack(p) for p in polys)), d_points)
    torch.cuda.synchronize()
    return out


def queries_of(count, seed):
    """`count` (polynomial, point) pairs: the first on the point 0, the second on the point 1, then random ones with repeats"""
    rnd = random.Random("queries %d %s" % (count, seed))
    qs = [(0, 0), (N_POLYS - 1, 1)][:count]
    while len(qs) < count:
        qs.append((rnd.randrange(N_POLYS), rnd.randrange(N_POINTS)))
    if count == 40:
        assert len(set(qs)) < count and {q[1] for q in qs} >= {0, 1}  # 40 pairs out of 15: some repeat
    return qs


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_eval_many_is_horner_and_the_bytes_of_eval_dev(gpu_ctx, pctx, shared, curve, n, count):
    import torch

    from snark_verifier_amd import poly, poly_batch

    ctx = pctx if curve == "pallas" else gpu_ctx
    values, d_polys, d_points = shared[curve, n]
    qs = queries_of(count, (curve, n))
    pad = 64
    d_out = torch.full((pad + 32 * count + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    d_one = torch.full((32 * count,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    poly_batch.eval_many_dev(ctx, d_polys, n, N_POLYS, d_points, N_POINTS, [q[0] for q in qs], [q[1] for q in qs], d_out.data_ptr() + pad)
    for i, (p, x) in enumerate(qs):
        poly.eval_dev(ctx, d_polys.data_ptr() + 32 * n * p, n, d_points.data_ptr() + 32 * x, d_one.data_ptr() + 32 * i)
    ctx.sync()
    raw, one = d_out.cpu().numpy().tobytes(), d_one.cpu().numpy().tobytes()
    assert raw[:pad] == b"\xa5" * pad and raw[pad + 32 * count:] == b"\xa5" * pad  # nothing written around the results
    got = [int.from_bytes(raw[pad + 32 * i:pad + 32 * i + 32], "little") for i in range(count)]
    assert got == [values[p][x] for p, x in qs], (curve, n, count)
    assert raw[pad:pad + 32 * count] == one


def test_a_count_above_the_grid_limit_runs_in_chunks(gpu_ctx):
    """65 600 queries of two short polynomials: one launch takes 65 535 of them (poly_batch.GRID_QUERIES), the rest a second"""
    import torch

    from snark_verifier_amd import poly_batch

    r, n, count = O.R, 2, 65600
    assert count > poly_batch.GRID_QUERIES
    rnd = random.Random("gpu-poly-batch-chunks")
    polys = [[rnd.randrange(r) for _ in range(n)] for _ in range(2)]
    points = [rnd.randrange(r) for _ in range(7)]
    qs = [(i % 2, (i * 3) % 7) for i in range(count)]
    d_polys, d_points = _dev(b"".join(_pack(p) for p in polys)), _dev(_pack(points))
    d_out = torch.full((32 * count + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    poly_batch.eval_many_dev(gpu_ctx, d_polys, n, 2, d_points, 7, [q[0] for q in qs], [q[1] for q in qs], d_out)
    gpu_ctx.sync()
    raw = d_out.cpu().numpy().tobytes()
    assert raw[32 * count:] == b"\xa5" * 64
    want = {(p, x): horner(polys[p], points[x], r) for p in range(2) for x in range(7)}
    assert raw[:32 * count] == b"".join(want[q].to_bytes(32, "little") for q in qs)
