"""GPU: the column products (snark_verifier_amd.poly_prod, include/snarkv_poly_prod.h) on BN254 and pallas against Python
integers, byte for byte on canonical words: the batch inversion and the grand product at lengths on both sides of one block of
the scans (poly_prod.BLOCK), of one block of blocks (BLOCK * LEVEL_BLOCK) and at a ragged three-level length, with zeros
planted at the ends, around a block boundary, over a whole block and as the words of r; the pointwise and the affine product
around one pass of terms; a permutation argument end to end; and the overlap refusals on a real context.

Nothing is filtered: every output is compared, the planted zeros included.  Inverses are checked by multiplication."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import pallas as PA  # noqa: E402

pytestmark = pytest.mark.gpu
FIELD = {"bn254": O.R, "pallas": PA.R}
GENERATOR = {"bn254": (7, 28), "pallas": (5, 32)}  # g and S of include/snarkv_ntt.h
B, B1 = 1024, 256  # poly_prod.BLOCK, poly_prod.LEVEL_BLOCK (asserted below)
# around one block, around one block of blocks (the last has three levels), and three levels ragged on each
LENGTHS = [1, 2, B - 1, B, B + 1, B * B1 - 1, B * B1, B * B1 + 1, B * B1 + 2 * B + 37]
MAX_N = max(LENGTHS)
GUARD = 64


@pytest.fixture(scope="module")
def P():
    from snark_verifier_amd import poly_prod

    assert (poly_prod.BLOCK, poly_prod.LEVEL_BLOCK, poly_prod.AFFINE_TERMS) == (B, B1, 16)
    return poly_prod


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


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ints(raw):
    if not isinstance(raw, (bytes, bytearray)):
        raw = _bytes(raw)
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _fresh(n_elems, guard=GUARD):
    """a buffer of 0xAA bytes with a guard behind it"""
    import torch

    return torch.full((32 * n_elems + guard,), 0xAA, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def shared():
    """per curve: 2 * MAX_N random non-zero values as integers, as bytes and on the device, and the prefix products of the
    first MAX_N -- computed once, never changed"""
    import torch

    out = {}
    for curve, r in FIELD.items():
        rnd = random.Random("gpu-poly-prod-" + curve)
        v = [rnd.randrange(1, r) for _ in range(2 * MAX_N)]
        prefix, acc = [], 1
        for x in v[:MAX_N]:
            prefix.append(acc)
            acc = acc * x % r
        prefix.append(acc)
        raw = _pack(v)
        out[curve] = (v, raw, _dev(raw), prefix, rnd.randrange(2, r))
    torch.cuda.synchronize()
    return out


def planted(n, r):
    """index -> value: zeros at 0 and n - 1, on both sides of the first block boundary, over the whole third block, and the
    words of r in the middle of what is left -- as far as n has these places"""
    z = {0: 0, n - 1: 0}
    if n > B:
        z[B - 1] = z[B] = 0
    for i in range(2 * B, min(3 * B, n)):
        z[i] = 0
    z[n // 2] = r
    return z


def _with(raw, n, changes):
    buf = bytearray(raw[:32 * n])
    for i, v in changes.items():
        buf[32 * i:32 * i + 32] = int(v).to_bytes(32, "little")
    return bytes(buf)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_batch_invert(P, ctx_of, shared, curve, n):
    import torch

    r, ctx = FIELD[curve], ctx_of(curve)
    v, raw = shared[curve][:2]
    for changes in ({}, planted(n, r)) if n > 2 else ({}, planted(n, r), {i: 0 for i in range(n)}):
        src = _with(raw, n, changes)
        d_in, d_out = _dev(src), _fresh(n)
        torch.cuda.synchronize()
        P.batch_invert_dev(ctx, d_in, n, d_out)
        ctx.sync()
        got = _bytes(d_out)
        assert got[32 * n:] == b"\xaa" * GUARD  # nothing behind out
        assert _bytes(d_in) == src
        for i, y in enumerate(_ints(got[:32 * n])):
            x = changes.get(i, v[i])
            assert y < r, i
            assert (y == 0) if x % r == 0 else (x * y % r == 1), (n, i)
        P.batch_invert_dev(ctx, d_in, n, d_in)  # in place: the same bytes
        ctx.sync()
        assert _bytes(d_in) == got[:32 * n]


def _grand(vals, start, r):
    out, acc = [], start
    for x in vals:
        out.append(acc)
        acc = acc * x % r
    return out, acc


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_grand_product(P, ctx_of, shared, curve, n):
    import torch

    r, ctx = FIELD[curve], ctx_of(curve)
    v, raw, d_v, prefix, s = shared[curve]
    d_small = _dev(_pack([s]) + b"\xaa" * (3 * 32 + GUARD))  # the start value, three totals, a guard
    d_a, d_b = _fresh(n), _fresh(n)
    torch.cuda.synchronize()
    small = d_small.data_ptr()
    P.grand_product_dev(ctx, d_v, n, d_a, d_total=small + 32)  # without a start value
    P.grand_product_dev(ctx, d_v, n, d_b, d_start=small, d_total=small + 64)
    ctx.sync()
    want = _pack(prefix[:n])
    assert _bytes(d_a) == want + b"\xaa" * GUARD
    assert _bytes(d_b) == _pack([s * p % r for p in prefix[:n]]) + b"\xaa" * GUARD
    totals = _ints(_bytes(d_small)[:128])
    assert totals[:3] == [s, prefix[n], s * prefix[n] % r]
    assert _bytes(d_small)[96:] == b"\xaa" * (32 + GUARD)
    # a zero factor in the middle (the words of r on pallas: zero all the same): later outputs and the total are zero,
    # earlier ones as before; then the same in place; then the total alone is looked at, with d_out given
    mid = n // 2
    src = _with(raw, n, {mid: r if curve == "pallas" else 0})
    d_f, d_c = _dev(src), _fresh(n)
    torch.cuda.synchronize()
    P.grand_product_dev(ctx, d_f, n, d_c, d_start=small, d_total=small + 96)
    ctx.sync()
    with_zero = _pack([s * p % r for p in prefix[:mid + 1]] + [0] * (n - mid - 1))
    assert _bytes(d_c) == with_zero + b"\xaa" * GUARD
    assert _ints(_bytes(d_small)[:128])[3] == 0
    assert _bytes(d_f) == src
    P.grand_product_dev(ctx, d_f, n, d_f, d_start=small)  # in place, no total
    ctx.sync()
    assert _bytes(d_f) == with_zero
    assert _bytes(d_small)[:128] == _pack([s, prefix[n], s * prefix[n] % r, 0])


@pytest.mark.parametrize("n", [1, 257, 65537])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_mul(P, ctx_of, shared, curve, n):
    import torch

    r, ctx = FIELD[curve], ctx_of(curve)
    v, raw, d_v = shared[curve][:3]
    a, b = v[:n], v[MAX_N:MAX_N + n]
    want = _pack([x * y % r for x, y in zip(a, b)])
    d_b = d_v.data_ptr() + 32 * MAX_N
    d_out = _fresh(n)
    torch.cuda.synchronize()
    P.mul_dev(ctx, d_v, d_b, n, d_out)
    ctx.sync()
    assert _bytes(d_out) == want + b"\xaa" * GUARD
    for first in (True, False):  # in place on either operand
        d_x, d_y = _dev(raw[:32 * n]), _dev(raw[32 * MAX_N:32 * (MAX_N + n)])
        torch.cuda.synchronize()
        P.mul_dev(ctx, d_x, d_y, n, d_x if first else d_y)
        ctx.sync()
        assert _bytes(d_x if first else d_y) == want
        assert _bytes(d_y if first else d_x) == (raw[32 * MAX_N:32 * (MAX_N + n)] if first else raw[:32 * n])
    d_m = _dev(_pack([r - 1] * n))  # (r - 1)^2 = 1, and the square of a column in place
    torch.cuda.synchronize()
    P.mul_dev(ctx, d_m, d_m, n, d_m)
    ctx.sync()
    assert _bytes(d_m) == _pack([1] * n)


@pytest.mark.parametrize("count", [1, 2, 16, 17])
@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_prod_affine(P, ctx_of, shared, curve, count):
    """count = 16 | 17 on both sides of one pass; terms with and without a beta part, repeated indices, beta and gamma from
    0, r - 1 and random values; and every column all r - 1 with beta = gamma = r - 1, the largest sums the bound meets"""
    import torch

    r, ctx = FIELD[curve], ctx_of(curve)
    v = shared[curve][0]
    rnd = random.Random("prod-affine-%s-%d" % (curve, count))
    for n in (1, 257, 2049):
        cols = [v[j * n:(j + 1) * n] for j in range(3)] + [[r - 1] * n]
        d_polys = _dev(_pack(sum(cols, [])))
        pick = lambda: rnd.choice([0, r - 1, rnd.randrange(r), rnd.randrange(r)])  # noqa: E731
        cases = [([rnd.randrange(4) for _ in range(count)], [rnd.choice([P.NONE, 0, 1, 2, 3]) for _ in range(count)],
                  [pick() for _ in range(count)], [pick() for _ in range(count)]),
                 ([3] * count, [3] * count, [r - 1] * count, [r - 1] * count),
                 ([3] * count, [P.NONE] * count, [r - 1] * count, [r - 1] * count)]
        cases[0][1][0] = P.NONE  # at least one term of each kind (count = 1: the one after this line)
        cases[0][1][-1] = 2
        for ia, ib, be, ga in cases:
            d_out = _fresh(n)
            torch.cuda.synchronize()
            P.prod_affine_dev(ctx, d_polys, n, 4, ia, ib, be, ga, d_out)
            ctx.sync()
            want = []
            for i in range(n):
                acc = 1
                for j in range(count):
                    acc = acc * (cols[ia[j]][i] + (be[j] * cols[ib[j]][i] if ib[j] != P.NONE else 0) + ga[j]) % r
                want.append(acc)
            assert _bytes(d_out) == _pack(want) + b"\xaa" * GUARD, (n, ia, ib)


def _permutation_instance(curve, k, n_cols, seed):
    """-> (w, delta, values, sigma labels): id_j[i] = delta^j w^i, sigma a seeded random permutation of the cells, the values
    constant on its cycles"""
    import ntt_util as U

    r = FIELD[curve]
    n = 1 << k
    g, s = GENERATOR[curve]
    w, delta = U.omega(curve, k), pow(g, 1 << s, r)
    assert pow(w, n, r) == 1 and pow(w, n // 2, r) == r - 1
    rnd = random.Random(seed)
    cells = list(range(n_cols * n))
    perm = list(cells)
    rnd.shuffle(perm)
    label = [pow(delta, c // n, r) * pow(w, c % n, r) % r for c in cells]
    values = [None] * len(cells)
    for c in cells:
        if values[c] is None:
            val = rnd.randrange(r)
            while values[c] is None:
                values[c] = val
                c = perm[c]
    sigma = [label[perm[c]] for c in cells]
    return w, delta, values, sigma, label


def _z_oracle(values, ids, sigmas, n, cols, beta, gamma, start, r):
    z, acc = [], start
    for i in range(n):
        z.append(acc)
        num = den = 1
        for j in cols:
            num = num * (values[j * n + i] + beta * ids[j * n + i] + gamma) % r
            den = den * (values[j * n + i] + beta * sigmas[j * n + i] + gamma) % r
        acc = acc * num % r * pow(den, -1, r) % r
    return z, acc


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_permutation_argument_end_to_end(P, ctx_of, shared, curve):
    import torch

    from snark_verifier_amd import ntt

    r, ctx = FIELD[curve], ctx_of(curve)
    k, m = 10, 3
    n = 1 << k
    w, delta, values, sigma, label = _permutation_instance(curve, k, m, "perm-%s" % curve)
    rnd = random.Random("perm-challenges-%s" % curve)
    beta, gamma = rnd.randrange(1, r), rnd.randrange(1, r)
    # on the CPU first: the argument holds for this seed, and does not with one cell changed
    z_want, total_want = _z_oracle(values, label, sigma, n, range(m), beta, gamma, 1, r)
    assert total_want == 1
    broken = list(values)
    broken[n + 17] = (broken[n + 17] + 1) % r
    z_broken, total_broken = _z_oracle(broken, label, sigma, n, range(m), beta, gamma, 1, r)
    assert total_broken != 1
    # columns on the device: 0..2 the values, 3..5 the identity (made by the forward transform of [0, delta^j, 0, ...]),
    # 6..8 sigma, 9..11 the broken values
    seeds = []
    for j in range(m):
        seeds += [0, pow(delta, j, r)] + [0] * (n - 2)
    d_polys = _dev(_pack(values) + _pack(seeds) + _pack(sigma) + _pack(broken))
    torch.cuda.synchronize()
    base = d_polys.data_ptr()
    ntt.ntt_dev(ctx, base + 32 * n * m, base + 32 * n * m, k, m)
    ctx.sync()
    assert _bytes(d_polys)[32 * n * m:32 * n * 2 * m] == _pack(label)
    iv, iid, isg = [0, 1, 2], [3, 4, 5], [6, 7, 8]
    d_work, d_z, d_tot = _fresh(2 * n), _fresh(n), _fresh(2)
    torch.cuda.synchronize()
    P.perm_product_dev(ctx, d_polys, n, 12, iv, iid, isg, beta, gamma, d_work, d_z, d_total=d_tot)
    ctx.sync()
    assert _bytes(d_z) == _pack(z_want) + b"\xaa" * GUARD
    assert _bytes(d_tot) == _pack([1]) + b"\xaa" * (32 + GUARD)
    z = _ints(_bytes(d_z)[:32 * n]) + [1]  # z(w^n) = z(1): the total closes the cycle
    for i in range(n):  # the constraint of the verifier, row by row
        left, right = z[i + 1], z[i]
        for j in range(m):
            left = left * (values[j * n + i] + beta * sigma[j * n + i] + gamma) % r
            right = right * (values[j * n + i] + beta * pow(delta, j, r) * pow(w, i, r) + gamma) % r
        assert left == right, i
    # one cell changed: the total is not 1
    d_tot2 = _fresh(1)
    torch.cuda.synchronize()
    P.perm_product_dev(ctx, d_polys, n, 12, [0, 10, 2], iid, isg, beta, gamma, d_work, d_z, d_total=d_tot2)
    ctx.sync()
    assert _ints(_bytes(d_tot2)[:32]) == [total_broken] and total_broken != 1
    assert _bytes(d_z)[:32 * n] == _pack(z_broken)
    # two chunks of columns, the second chained to the first through its last row (halo2's permutation sets)
    d_z1, d_z2, d_t = _fresh(n), _fresh(n), _fresh(2)
    torch.cuda.synchronize()
    P.perm_product_dev(ctx, d_polys, n, 12, iv[:2], iid[:2], isg[:2], beta, gamma, d_work, d_z1, d_total=d_t)
    P.perm_product_dev(ctx, d_polys, n, 12, iv[2:], iid[2:], isg[2:], beta, gamma, d_work, d_z2,
                       d_start=d_z1.data_ptr() + 32 * (n - 1), d_total=d_t.data_ptr() + 32)
    ctx.sync()
    z1_want, t1 = _z_oracle(values, label, sigma, n, [0, 1], beta, gamma, 1, r)
    z2_want, t2 = _z_oracle(values, label, sigma, n, [2], beta, gamma, z1_want[n - 1], r)
    assert _bytes(d_z1) == _pack(z1_want) + b"\xaa" * GUARD and _bytes(d_z2) == _pack(z2_want) + b"\xaa" * GUARD
    assert _bytes(d_t) == _pack([t1, t2]) + b"\xaa" * GUARD
    # the four public calls, made separately, give the same bytes (work included)
    d_w2, d_z3, d_t3 = _fresh(2 * n), _fresh(n), _fresh(1)
    torch.cuda.synchronize()
    num, den = d_w2.data_ptr(), d_w2.data_ptr() + 32 * n
    P.prod_affine_dev(ctx, d_polys, n, 12, iv, iid, [beta] * m, [gamma] * m, num)
    P.prod_affine_dev(ctx, d_polys, n, 12, iv, isg, [beta] * m, [gamma] * m, den)
    P.batch_invert_dev(ctx, den, n, den)
    P.mul_dev(ctx, num, den, n, num)
    P.grand_product_dev(ctx, num, n, d_z3, d_total=d_t3)
    P.perm_product_dev(ctx, d_polys, n, 12, iv, iid, isg, beta, gamma, d_work, d_z, d_total=d_tot)
    ctx.sync()
    assert _bytes(d_z3) == _bytes(d_z) == _pack(z_want) + b"\xaa" * GUARD
    assert _bytes(d_w2) == _bytes(d_work) and _bytes(d_t3)[:32] == _bytes(d_tot)[:32] == _pack([1])


@pytest.mark.parametrize("curve", ["bn254", "pallas"])
def test_overlap_is_refused_and_nothing_is_written(P, ctx_of, shared, curve):
    import torch

    import snark_verifier_amd as sv

    r, ctx = FIELD[curve], ctx_of(curve)
    v, raw, _, prefix, s = shared[curve]
    n = 1500
    src = raw[:32 * 3 * n]
    d_p = _dev(src)  # three columns
    d_o = _fresh(2 * n)
    torch.cuda.synchronize()
    p, o = d_p.data_ptr(), d_o.data_ptr()
    refused = [
        lambda: P.mul_dev(ctx, p, p + 32 * n, n, p + 32),
        lambda: P.mul_dev(ctx, p, p + 32 * n, n, p + 32 * n - 32),
        lambda: P.batch_invert_dev(ctx, p, n, p + 32),
        lambda: P.batch_invert_dev(ctx, p + 32, n, p),
        lambda: P.grand_product_dev(ctx, p, n, p + 32 * (n - 1)),
        lambda: P.grand_product_dev(ctx, p, n, o, d_total=o + 32),
        lambda: P.grand_product_dev(ctx, p, n, o, d_total=p + 64),
        lambda: P.grand_product_dev(ctx, p, n, o, d_start=o + 32 * (n - 1)),
        lambda: P.grand_product_dev(ctx, p, n, p, d_start=p),
        lambda: P.prod_affine_dev(ctx, p, n, 3, [0, 1], [P.NONE, 2], [1, 1], [1, 1], p + 32 * 2 * n + 32 * (n - 1)),
        lambda: P.prod_affine_dev(ctx, p, n, 3, [0], [P.NONE], [1], [1], p - 32 * (n - 1)),
        lambda: P.perm_product_dev(ctx, p, n, 3, [0], [1], [2], 3, 5, o, p + 32 * n),
        lambda: P.perm_product_dev(ctx, p, n, 3, [0], [1], [2], 3, 5, p + 32 * 2 * n, o),
        lambda: P.perm_product_dev(ctx, p, n, 3, [0], [1], [1], 3, 5, o, o + 32 * n),
        lambda: P.perm_product_dev(ctx, p, n, 2, [0], [1], [1], 3, 5, o, p + 32 * 2 * n, d_total=o + 32 * n),
        lambda: P.perm_product_dev(ctx, p, n, 2, [0], [1], [1], 3, 5, o, p + 32 * 2 * n, d_start=o),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(sv.SnarkvError) as e:
            call()
        assert e.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(e.value), i
    ctx.sync()
    assert _bytes(d_p) == src and _bytes(d_o) == b"\xaa" * (32 * 2 * n + GUARD)
    # the context stays usable, and what is allowed is: a start value inside the factors, out elsewhere
    P.grand_product_dev(ctx, p, n, o, d_start=p + 32 * 5, d_total=o + 32 * n)
    ctx.sync()
    want, total = _grand(v[:n], v[5], r)
    assert _bytes(d_o)[:32 * (n + 1)] == _pack(want + [total])
    assert _bytes(d_o)[32 * (n + 1):] == b"\xaa" * (32 * (n - 1) + GUARD)
