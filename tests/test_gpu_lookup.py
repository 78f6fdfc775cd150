"""GPU: the lookup argument (snark_verifier_amd.lookup, include/snarkv_lookup.h) on BN254 and pallas against Python integers
(tests/lookup_util.py), byte for byte on canonical words with nothing filtered: the sort at lengths around one tile, at an odd
number of runs with a ragged end and at many chunks per merge, on inputs with long ties, keys that differ in one word only and
values at and above r, out of place and in place; halo2's permute_expression_pair against the sequential model, the status
included, and against the reference's constraints recomputed in integers; the lookup product against the four separate calls
of snarkv_poly_prod.h; and one lookup end to end through the quotient's gate program.

Outputs sit in 0xAA-filled buffers with a guard behind them, which must be intact."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lookup_util as LU  # noqa: E402
import quotient_util as QU  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "pallas"]
T = 1024  # lookup.TILE = lookup.SCAN_BLOCK (asserted below)
# around one tile; two tiles (one pass) and one more element (two passes, the third run carried over); three passes with an
# odd run count and a ragged end; many chunks per merge
SORT_LENGTHS = [1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T - 1, 5 * T + 3, 64 * T + T // 2 + 1]
PERMUTE_ROWS = [1, T - 1, T + 1, 3 * T - 1, 5 * T + 3]
PRODUCT_LENGTHS = [1, T + 1, 5 * T + 3]
GUARD = 64
_pack, _ints = LU.pack, LU.unpack


@pytest.fixture(scope="module")
def L():
    from snark_verifier_amd import lookup

    assert (lookup.TILE, lookup.SCAN_BLOCK, lookup.SCAN_LEVEL_BLOCK) == (T, T, T)
    return lookup


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


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _fresh(n_elems, guard=GUARD):
    """a buffer of 0xAA bytes with a guard behind it"""
    import torch

    return torch.full((32 * n_elems + guard,), 0xAA, dtype=torch.uint8, device="cuda")


def _sync():
    import torch

    torch.cuda.synchronize()


def _intact(t, n_elems, guard=GUARD):
    """the first n_elems elements of a _fresh buffer; what lies behind them is still 0xAA"""
    raw = _bytes(t)
    assert raw[32 * n_elems:] == b"\xaa" * (len(raw) - 32 * n_elems)
    return raw[:32 * n_elems]


@pytest.mark.parametrize("n", SORT_LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_sort(L, ctx_of, curve, n):
    r, ctx = LU.FIELD[curve], ctx_of(curve)
    for name, vals in LU.sort_inputs(n, r, curve).items():
        src = _pack(vals)
        want = _pack(LU.sort_model(vals, r))
        d_in, d_work, d_out = _dev(src), _fresh(n), _fresh(n)
        _sync()
        L.sort_dev(ctx, d_in, n, d_work, d_out)
        ctx.sync()
        assert _intact(d_out, n) == want, name
        _intact(d_work, n)
        assert _bytes(d_in) == src
        L.sort_dev(ctx, d_in, n, d_work, d_in)  # in place
        ctx.sync()
        assert _bytes(d_in) == want, name
        _intact(d_work, n)


def _permute(L, ctx, A, S, u, rows):
    """the call over the first u of `rows` rows -> (A', S', status) as integers; rows from u on and the guards are checked"""
    d_a, d_s = _dev(_pack(A)), _dev(_pack(S))
    d_work, d_pi, d_pt, d_st = _fresh(2 * u), _fresh(rows), _fresh(rows), _fresh(1)
    _sync()
    L.permute_dev(ctx, d_a, d_s, u, d_work, d_pi, d_pt, d_st)
    ctx.sync()
    assert _bytes(d_a) == _pack(A) and _bytes(d_s) == _pack(S)
    _intact(d_work, 2 * u)
    st = _bytes(d_st)
    assert st[16:] == b"\xaa" * (16 + GUARD)
    status = [int.from_bytes(st[4 * i:4 * i + 4], "little") for i in range(4)]
    return _ints(_intact(d_pi, u)), _ints(_intact(d_pt, u)), status  # rows >= u still 0xAA


@pytest.mark.parametrize("u", PERMUTE_ROWS)
@pytest.mark.parametrize("curve", CURVES)
def test_permute(L, ctx_of, curve, u):
    r, ctx = LU.FIELD[curve], ctx_of(curve)
    cases = LU.permute_cases(u, r, T, T, curve)
    if u > T:
        assert {"shuffle", "constant input", "range table", "multiplicities", "run over tile border", "run over scan border",
                "1 missing", "7 missing"} <= set(cases)
    for name, (A, S, missing) in cases.items():
        rows = u + 6  # the caller's blinding rows lie behind the u usable ones
        A, S = A + [0xAA] * 6, S + [0xAA] * 6
        want = LU.permute_model(A, S, u, r)
        got = _permute(L, ctx, A, S, u, rows)
        assert got[2] == want[2] and want[2][0] == missing, (name, got[2])
        assert got[0] == want[0], name
        assert got[1] == want[1], name
        # the reference's constraints on what the device wrote, in integers
        assert LU.constraints_hold(A, S, got[0], got[1], u, r) == (missing == 0), name


def _satisfied(curve, n):
    """A, S, A', S' of a satisfied lookup over n rows (no blinding rows): a table with repeats, some values unused"""
    r = LU.FIELD[curve]
    rnd = random.Random("lookup-product-%s-%d" % (curve, n))
    table = [rnd.randrange(r) for _ in range(max(n // 3, 1))]
    S = (table * (n // len(table) + 1))[:n]
    A = [rnd.choice(table[:max(len(table) // 2, 1)]) for _ in range(n)]
    rnd.shuffle(S)
    A1, S1, status = LU.permute_model(A, S, n, r)
    assert status[0] == 0
    return A, S, A1, S1, rnd


@pytest.mark.parametrize("n", PRODUCT_LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_product(L, ctx_of, curve, n):
    from snark_verifier_amd import poly_prod as P

    r, ctx = LU.FIELD[curve], ctx_of(curve)
    A, S, _, _, rnd = _satisfied(curve, n)
    beta, gamma = rnd.randrange(1, r), rnd.randrange(1, r)
    # the permuted columns come from the device: columns 0 A, 1 S, 2 A', 3 S', 4 S' with two entries swapped for others
    d_polys = _dev(_pack(A) + _pack(S) + b"\xaa" * (32 * 3 * n))
    d_pw, d_st = _fresh(2 * n), _fresh(1)
    base = d_polys.data_ptr()
    _sync()
    L.permute_dev(ctx, base, base + 32 * n, n, d_pw, base + 64 * n, base + 96 * n, d_st)
    ctx.sync()
    cols = _ints(_bytes(d_polys))
    A1, S1 = cols[2 * n:3 * n], cols[3 * n:4 * n]
    assert (A1, S1) == LU.permute_model(A, S, n, r)[:2] and _bytes(d_st)[:16] == bytes(4) + (len(set(A))).to_bytes(4, "little") + bytes(8)
    bad = list(S1)
    bad[0], bad[n - 1] = (bad[0] + 1) % r, (bad[n - 1] + 2) % r
    d_polys[32 * 4 * n:] = _dev(_pack(bad))
    d_work, d_z, d_tot = _fresh(2 * n), _fresh(n), _fresh(2)
    _sync()
    L.product_dev(ctx, d_polys, n, 5, 0, 1, 2, 3, beta, gamma, d_work, d_z, d_total=d_tot)
    ctx.sync()
    z_want, total = LU.product_model(A, S, A1, S1, beta, gamma, 1, r)
    assert total == 1
    assert _intact(d_z, n) == _pack(z_want) and _intact(d_tot, 1) == _pack([1])
    # the four public calls, made separately, give the same bytes (work included)
    d_w2, d_z2, d_t2 = _fresh(2 * n), _fresh(n), _fresh(1)
    _sync()
    num, den = d_w2.data_ptr(), d_w2.data_ptr() + 32 * n
    P.prod_affine_dev(ctx, d_polys, n, 5, [0, 1], [P.NONE, P.NONE], [0, 0], [beta, gamma], num)
    P.prod_affine_dev(ctx, d_polys, n, 5, [2, 3], [P.NONE, P.NONE], [0, 0], [beta, gamma], den)
    P.batch_invert_dev(ctx, den, n, den)
    P.mul_dev(ctx, num, den, n, num)
    P.grand_product_dev(ctx, num, n, d_z2, d_total=d_t2)
    ctx.sync()
    assert _bytes(d_z2) == _bytes(d_z) and _bytes(d_w2) == _bytes(d_work) and _bytes(d_t2)[:32] == _pack([1])
    # two entries of S' swapped for others: the total is not one
    d_z3, d_t3 = _fresh(n), _fresh(1)
    _sync()
    L.product_dev(ctx, d_polys, n, 5, 0, 1, 2, 4, beta, gamma, d_work, d_z3, d_total=d_t3)
    ctx.sync()
    z_bad, total_bad = LU.product_model(A, S, A1, bad, beta, gamma, 1, r)
    assert total_bad != 1 and _intact(d_z3, n) == _pack(z_bad) and _intact(d_t3, 1) == _pack([total_bad])
    # chained: a second lookup starts from the last row of the first one's z, and needs no total
    start = z_want[n - 1]
    d_z4 = _fresh(n)
    _sync()
    L.product_dev(ctx, d_polys, n, 5, 1, 0, 3, 2, gamma, beta, d_work, d_z4, d_start=d_z.data_ptr() + 32 * (n - 1))
    ctx.sync()
    assert _intact(d_z4, n) == _pack(LU.product_model(S, A, S1, A1, gamma, beta, start, r)[0])
    assert _intact(d_z, n) == _pack(z_want)


@pytest.mark.parametrize("curve", CURVES)
def test_one_lookup_through_the_quotient_gate_program(L, ctx_of, curve):
    """n = 2^11 rows of which u = n - 6 are usable: A' and S' from permute_dev, z from product_dev over the u rows with its
    total stored at row u, and the two reference constraints evaluated by quotient_eval_dev (e = 0) on the columns
    0 A, 1 S, 2 A', 3 S', 4 z: zero on every usable row"""
    import torch

    from snark_verifier_amd import quotient as Q

    r, ctx, k = LU.FIELD[curve], ctx_of(curve), 11
    n = 1 << k
    u = n - 6
    A, S, _, _, rnd = _satisfied(curve, u)
    beta, gamma = rnd.randrange(1, r), rnd.randrange(1, r)
    blind = lambda: [rnd.randrange(r) for _ in range(n - u)]  # noqa: E731
    d_cols = _dev(_pack(A + blind()) + _pack(S + blind()) + _pack([0] * u + blind()) + _pack([0] * u + blind())
                  + _pack([0] * u + blind()))
    src = _bytes(d_cols)
    col = [d_cols.data_ptr() + 32 * n * j for j in range(5)]
    d_pw, d_st = _fresh(2 * u), _fresh(1)
    _sync()
    L.permute_dev(ctx, col[0], col[1], u, d_pw, col[2], col[3], d_st)
    ctx.sync()
    # the product runs over the u usable rows: its columns are u elements apart
    d_packed = torch.cat([d_cols[32 * n * j:32 * n * j + 32 * u] for j in range(4)])
    d_work = _fresh(2 * u)
    _sync()
    L.product_dev(ctx, d_packed, u, 4, 0, 1, 2, 3, beta, gamma, d_work, col[4], d_total=col[4] + 32 * u)
    ctx.sync()
    got = _bytes(d_cols)
    assert _bytes(d_st)[:4] == bytes(4)
    for j in range(5):  # the blinding rows are the caller's: only z's first takes the total
        keep = 32 * (u + 1) if j == 4 else 32 * u
        assert got[32 * n * j + keep:32 * n * (j + 1)] == src[32 * n * j + keep:32 * n * (j + 1)], j
    cols = _ints(got)
    A1, S1, z = cols[2 * n:2 * n + u], cols[3 * n:3 * n + u], cols[4 * n:4 * n + u + 1]
    assert (A1, S1) == LU.permute_model(A, S, u, r)[:2] and z[0] == 1 and z[u] == 1
    # z(wX) (A' + beta)(S' + gamma) - z (A + beta)(S + gamma)
    p1 = Q.Program()
    b, g = p1.const(beta), p1.const(gamma)
    p1.add(0, Q.COL(2), b)
    p1.add(1, Q.COL(3), g)
    p1.mul(0, Q.REG(0), Q.REG(1))
    p1.mul(0, Q.REG(0), Q.COL(4, 1))
    p1.add(1, Q.COL(0), b)
    p1.add(2, Q.COL(1), g)
    p1.mul(1, Q.REG(1), Q.REG(2))
    p1.mul(1, Q.REG(1), Q.COL(4))
    p1.sub(0, Q.REG(0), Q.REG(1))
    # (A' - S')(A' - A'(w^-1 X))
    p2 = Q.Program()
    p2.sub(0, Q.COL(2), Q.COL(3))
    p2.sub(1, Q.COL(2), Q.COL(2, -1))
    p2.mul(0, Q.REG(0), Q.REG(1))
    d_o1, d_o2 = _fresh(n), _fresh(n)
    _sync()
    Q.eval_dev(ctx, d_cols, k, 0, 5, p1, d_o1)
    Q.eval_dev(ctx, d_cols, k, 0, 5, p2, d_o2)
    ctx.sync()
    o1, o2 = _intact(d_o1, n), _intact(d_o2, n)
    assert o1 == bytes(QU.pack(QU.interpret(curve, [cols[n * j:n * (j + 1)] for j in range(5)], k, 0, p1.instrs, p1.consts)))
    assert o1[:32 * u] == bytes(32 * u)  # the product rule on every usable row
    assert o2[32:32 * u] == bytes(32 * (u - 1)) and o2[:32] == bytes(32)  # the second on rows 1 .. u - 1; row 0 by A'[0] = S'[0]
    assert o1[32 * u:] != bytes(32 * (n - u))  # the blinding rows are not constrained, and are not zero by accident
