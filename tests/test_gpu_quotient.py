"""GPU: the quotient calls (snark_verifier_amd.quotient, include/snarkv_quotient.h) on BN254 and pallas against Python
integers (tests/quotient_util.py), byte for byte on canonical words: the extension to the coset on both sides of the transform's
one-tile path, the gate program from one row to several workgroups (each op alone, a chain of 4096, all 16 registers,
rotations that wrap once and many times, the largest operands, one column in every operand), the division by the vanishing
polynomial in place and out of place, a small circuit end to end with its Z from poly_perm_product_dev and two broken
witnesses, and the overlap refusals on a real context.

Nothing is filtered: every output buffer starts as 0xAA bytes with a guard behind it, and the whole of it is compared."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quotient_util as QU  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "pallas"]
# k + e = 9 | 10: the two sides of the transform's one-tile path
SHAPES = [(0, 0), (0, 3), (1, 1), (3, 2), (8, 1), (8, 2), (7, 3)]
GUARD = 64
_pack, _ints = QU.pack, QU.unpack


@pytest.fixture(scope="module")
def Q():
    from snark_verifier_amd import quotient

    return quotient


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


@pytest.fixture(scope="module")
def shared():
    """per curve: 3 * 2^10 random values as integers -- computed once, never changed"""
    out = {}
    for curve, r in QU.FIELD.items():
        rnd = random.Random("gpu-quotient-" + curve)
        out[curve] = [rnd.randrange(r) for _ in range(3 << 10)]
    return out


# ---------------------------------------------------------------- extend
@pytest.mark.parametrize("k,e", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_extend(Q, ctx_of, shared, curve, k, e):
    from snark_verifier_amd import ntt

    ctx, s = ctx_of(curve), QU.zeta(curve)
    n, n_ext = 1 << k, 1 << (k + e)
    for count in (1, 3):
        polys = [shared[curve][p * n:(p + 1) * n] for p in range(count)]
        src = _pack(sum(polys, []))
        d_in, d_out, d_pad = _dev(src), _fresh(count * n_ext), _dev(_pack(sum((p + [0] * (n_ext - n) for p in polys), [])))
        _sync()
        Q.extend_dev(ctx, d_in, k, e, count, s, d_out)
        ntt.ntt_dev(ctx, d_pad, d_pad, k + e, count, shift=s)  # padding by hand and the transform
        ctx.sync()
        want = _pack(sum((QU.extend(curve, p, k, e, s) for p in polys), []))
        assert _bytes(d_out) == want + b"\xaa" * GUARD, count
        assert _bytes(d_pad) == want and _bytes(d_in) == src


# ---------------------------------------------------------------- eval
def _run_eval(Q, ctx, curve, cols, k, e, instrs, consts):
    """-> the output's integers; the guard and the columns are checked here"""
    n_ext = 1 << (k + e)
    src = _pack(sum(cols, []))
    d_cols, d_out = _dev(src), _fresh(n_ext)
    _sync()
    Q.eval_dev(ctx, d_cols, k, e, len(cols), (QU.pack_program(Q, instrs), consts), d_out)
    ctx.sync()
    got = _bytes(d_out)
    assert got[32 * n_ext:] == b"\xaa" * GUARD and _bytes(d_cols) == src
    return _ints(got[:32 * n_ext])


def _reverse_program(Q):
    """writes all 16 registers, then reads them in reverse"""
    c0, c1 = Q.COL(0), Q.COL(1, 1)
    instrs = [(QU.ADD, 0, c0, c1, 0)]
    for i in range(1, 16):
        instrs.append(((QU.ADD, QU.SUB, QU.MUL)[i % 3], i, Q.REG(i - 1), Q.COL(i % 2, i - 8), 0))
    for i in range(15, 0, -1):  # r15 = r15 r14 + r13, r14 = r14 r13 + r12, ..., r1 = r1 r0 + r15
        instrs.append((QU.FMA, i, Q.REG(i), Q.REG(i - 1), Q.REG((i - 2) % 16)))
    instrs.append((QU.SUB, 0, Q.REG(1), Q.REG(0), 0))
    return instrs


# N = 1, 2, 8 (below a wave), 2^10 (one workgroup of rows is 256: several), 2^12 with e = 8
@pytest.mark.parametrize("k,e", [(0, 0), (0, 1), (1, 2), (8, 2), (4, 8)])
@pytest.mark.parametrize("curve", CURVES)
def test_eval_programs(Q, ctx_of, shared, curve, k, e):
    r, ctx, n_ext = QU.FIELD[curve], ctx_of(curve), 1 << (k + e)
    v = shared[curve]
    cols = [[v[(p * n_ext + i) % len(v)] for i in range(n_ext)] for p in range(2)]
    consts = [v[5], r - 1, 0]
    c0, c1, k0 = Q.COL(0), Q.COL(1), Q.CONST(0)
    programs = {op: [(op, 7, c0, c1, k0 if op == QU.FMA else 0)] for op in (QU.ADD, QU.SUB, QU.MUL, QU.FMA)}  # each op alone
    programs["reverse"] = _reverse_program(Q)
    # +1 / -1: row N - 1 reads row 0 and row 0 reads row N - 1 (times 2^e)
    programs["rotations"] = [(QU.SUB, 0, Q.COL(0, 1), Q.COL(0, -1), 0), (QU.FMA, 0, Q.REG(0), Q.COL(1, -1), Q.COL(1, 1))]
    programs["one column everywhere"] = [(QU.FMA, 3, c1, c1, c1), (QU.FMA, 3, Q.REG(3), Q.REG(3), Q.REG(3))]
    rnd = random.Random("gpu-quotient-programs-%s-%d-%d" % (curve, k, e))
    programs["random"] = QU.random_program(Q, rnd, 48, 2, 3)
    for name, instrs in programs.items():
        assert _run_eval(Q, ctx, curve, cols, k, e, instrs, consts) == QU.interpret(curve, cols, k, e, instrs, consts), name


@pytest.mark.parametrize("curve", CURVES)
def test_eval_a_chain_of_4096(Q, ctx_of, shared, curve):
    """N = 2^10, the longest program: r0 = r0 * col + const, 4095 times.  The column repeats its first 8 values and the program
    has no rotation, so row i is row i mod 8 of the same program over 8 rows, which is what the integers run."""
    ctx, k, e = ctx_of(curve), 8, 2
    v = shared[curve]
    instrs = [(QU.ADD, 0, Q.COL(0), Q.CONST(0), 0)] + [(QU.FMA, 0, Q.REG(0), Q.COL(0), Q.CONST(1))] * (Q.MAX_INSTR - 1)
    consts = [v[8], v[9]]
    got = _run_eval(Q, ctx, curve, [[v[i % 8] for i in range(1 << (k + e))]], k, e, instrs, consts)
    small = QU.interpret(curve, [v[:8]], 3, 0, instrs, consts)
    assert got == [small[i % 8] for i in range(1 << (k + e))]


@pytest.mark.parametrize("curve", CURVES)
def test_eval_rotations_that_wrap_many_times(Q, ctx_of, shared, curve):
    """k = 3: -512 and 511 domain steps wrap 64 times; with e = 2 the step is four rows"""
    ctx, v = ctx_of(curve), shared[curve]
    for k, e in ((3, 0), (3, 2)):
        n_ext = 1 << (k + e)
        cols = [v[:n_ext], v[n_ext:2 * n_ext]]
        instrs = [(QU.MUL, 1, Q.COL(0, -512), Q.COL(1, 511), 0), (QU.ADD, 2, Q.COL(1, -512), Q.COL(0, 511), 0),
                  (QU.FMA, 0, Q.REG(1), Q.COL(0, 3), Q.REG(2)), (QU.SUB, 0, Q.REG(0), Q.COL(1, -5), 0)]
        assert _run_eval(Q, ctx, curve, cols, k, e, instrs, []) == QU.interpret(curve, cols, k, e, instrs, [])


@pytest.mark.parametrize("curve", CURVES)
def test_eval_at_the_largest_operands(Q, ctx_of, curve):
    """every column and constant r - 1; columns holding the words of r and of 2^256 - 1 (taken mod r)"""
    r, ctx, k, e = QU.FIELD[curve], ctx_of(curve), 5, 1
    n_ext = 1 << (k + e)
    c0, c1, k0 = Q.COL(0, 1), Q.COL(1, -1), Q.CONST(0)
    instrs = [(QU.ADD, 0, c0, k0, 0), (QU.SUB, 1, Q.CONST(1), c1, 0), (QU.SUB, 2, Q.REG(1), c0, 0), (QU.ADD, 3, Q.REG(0), Q.REG(0), 0),
              (QU.FMA, 4, Q.REG(3), Q.REG(2), Q.REG(3)), (QU.MUL, 5, c0, c1, 0), (QU.FMA, 6, c0, k0, c1),
              (QU.SUB, 4, Q.REG(2), Q.REG(4), 0), (QU.FMA, 4, Q.REG(4), Q.REG(6), Q.REG(5)), (QU.MUL, 4, Q.REG(4), Q.REG(4), 0),
              (QU.FMA, 0, Q.REG(4), Q.REG(0), Q.REG(1))]
    for cols in ([[r - 1] * n_ext] * 2, [[r] * n_ext, [(1 << 256) - 1] * n_ext], [[(1 << 256) - 1] * n_ext, [r - 1] * n_ext]):
        consts = [r - 1, 0]
        for upto in range(1, len(instrs) + 1):  # the result of every instruction in turn
            got = _run_eval(Q, ctx, curve, cols, k, e, instrs[:upto], consts)
            assert got == QU.interpret(curve, cols, k, e, instrs[:upto], consts), upto


# ---------------------------------------------------------------- div_vanishing
@pytest.mark.parametrize("k,e", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_div_vanishing(Q, ctx_of, shared, curve, k, e):
    r, ctx, s = QU.FIELD[curve], ctx_of(curve), QU.zeta(curve)
    n, n_ext = 1 << k, 1 << (k + e)
    vals = shared[curve][:n_ext]
    src = _pack(vals)
    d_in, d_out = _dev(src), _fresh(n_ext)
    _sync()
    Q.div_vanishing_dev(ctx, d_in, k, e, s, d_out)
    ctx.sync()
    got = _bytes(d_out)
    assert got[32 * n_ext:] == b"\xaa" * GUARD and _bytes(d_in) == src
    w_ext = QU.U.omega(curve, k + e)
    for i, y in enumerate(_ints(got[:32 * n_ext])):  # multiplied back, row by row
        assert y < r and y * (pow(s * pow(w_ext, i, r), n, r) - 1) % r == vals[i], i
    assert got[:32 * n_ext] == _pack(QU.div_vanishing(curve, vals, k, e, s))
    if e == 0:  # the constant divisor
        assert len(QU.vanishing_table(curve, k, e, s)) == 1
    Q.div_vanishing_dev(ctx, d_in, k, e, s, d_in)  # in place: the same bytes
    ctx.sync()
    assert _bytes(d_in) == got[:32 * n_ext]


# ---------------------------------------------------------------- quotient_dev, end to end
def _device_z(ctx, c):
    """the circuit's Z from poly_perm_product_dev -> (the tensor that holds it, its integers, the total)"""
    from snark_verifier_amd import poly_prod

    n = c.n
    d_polys = _dev(_pack(c.a + c.b + c.c + sum(c.ids, []) + sum(c.sigma, [])))
    d_work, d_z, d_total = _fresh(2 * n), _fresh(n), _fresh(1)
    _sync()
    poly_prod.perm_product_dev(ctx, d_polys, n, 9, [0, 1, 2], [3, 4, 5], [6, 7, 8], c.beta, c.gamma, d_work, d_z, d_total=d_total)
    ctx.sync()
    return d_z, _ints(_bytes(d_z)[:32 * n]), _ints(_bytes(d_total)[:32])[0]


def _device_coeffs(ctx, c, d_z):
    """the COLS coefficient columns on the device: the value columns (Z copied on the device) through the inverse transform, and
    the polynomial X"""
    from snark_verifier_amd import ntt

    n = c.n
    vals = c.value_columns([0] * n)
    d_coeffs = _dev(_pack(sum(vals, []) + [0, 1] + [0] * (n - 2)))
    d_coeffs[32 * n * QU.COL_Z:32 * n * (QU.COL_Z + 1)] = d_z[:32 * n]
    _sync()
    ntt.intt_dev(ctx, d_coeffs, d_coeffs, c.k, QU.COLS - 1)
    ctx.sync()
    return d_coeffs


def _device_eval(ctx, d_coeffs, n, x):
    """p(x) through poly_eval_dev"""
    from snark_verifier_amd import poly

    d_small = _dev(_pack([x]) + b"\xaa" * 32)
    _sync()
    poly.eval_dev(ctx, d_coeffs, n, d_small.data_ptr(), d_small.data_ptr() + 32)
    ctx.sync()
    return _ints(_bytes(d_small))[1]


@pytest.mark.parametrize("bad", [None, "gate", "copy"])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_of_the_small_circuit(Q, ctx_of, curve, bad):
    from snark_verifier_amd import ntt

    r, ctx, k, e = QU.FIELD[curve], ctx_of(curve), 4, 2
    n, n_ext, s = 1 << k, 1 << (k + e), QU.zeta(curve)
    s_inv = pow(s, -1, r)
    c = QU.Circuit(curve, k, bad)
    d_z, z, total = _device_z(ctx, c)
    assert (z, total) == c.z() and (total == 1) == (bad != "copy")
    d_coeffs = _device_coeffs(ctx, c, d_z)
    coeffs = c.coeff_columns(z)
    src = _pack(sum(coeffs, []))
    assert _bytes(d_coeffs) == src
    p = c.program(Q)
    d_work, d_h = _fresh(QU.COLS * n_ext), _fresh(n_ext)
    _sync()
    Q.quotient_dev(ctx, d_coeffs, k, e, QU.COLS, p, s, s_inv, d_work, d_h)
    ctx.sync()
    h = QU.quotient(curve, coeffs, k, e, p.instrs, p.consts, s)
    assert _bytes(d_h) == _pack(h) + b"\xaa" * GUARD  # the integer model, byte for byte
    assert _bytes(d_work)[32 * QU.COLS * n_ext:] == b"\xaa" * GUARD and _bytes(d_coeffs) == src
    # the four separate calls give the same bytes, work included
    d_work2, d_h2 = _fresh(QU.COLS * n_ext), _fresh(n_ext)
    _sync()
    Q.extend_dev(ctx, d_coeffs, k, e, QU.COLS, s, d_work2)
    Q.eval_dev(ctx, d_work2, k, e, QU.COLS, p, d_h2)
    Q.div_vanishing_dev(ctx, d_h2, k, e, s, d_h2)
    ntt.intt_dev(ctx, d_h2, d_h2, k + e, 1, shift=s_inv)
    ctx.sync()
    assert _bytes(d_h2) == _bytes(d_h) and _bytes(d_work2) == _bytes(d_work)
    # the degree bound and the identity h(x) (x^n - 1) = expr(x), every side through poly_eval_dev
    assert all(v == 0 for v in h[3 * n - 3:]) == (bad is None)
    x = random.Random("gpu-quotient-point-" + curve).randrange(r)
    values = [_device_eval(ctx, d_coeffs.data_ptr() + 32 * n * j, n, x) for j in range(10)]
    z_next = _device_eval(ctx, d_coeffs.data_ptr() + 32 * n * QU.COL_Z, n, x * c.w % r)
    h_x = _device_eval(ctx, d_h, n_ext, x)
    assert values == [QU.horner(cf, x, r) for cf in coeffs[:10]] and h_x == QU.horner(h, x, r)
    assert (h_x * (pow(x, n, r) - 1) % r == c.expression_of(x, values, z_next)) == (bad is None)
    if bad is None:  # the gate alone at e = 1: degree 3, h below 2n
        g = c.program(Q, permutation=False)
        d_work3, d_h3 = _fresh(QU.COLS * 2 * n), _fresh(2 * n)
        _sync()
        Q.quotient_dev(ctx, d_coeffs, k, 1, QU.COLS, g, s, s_inv, d_work3, d_h3)
        ctx.sync()
        hg = QU.quotient(curve, coeffs, k, 1, g.instrs, g.consts, s)
        assert _bytes(d_h3) == _pack(hg) + b"\xaa" * GUARD and all(v == 0 for v in hg[2 * n - 2:])
        hg_x = _device_eval(ctx, d_h3, 2 * n, x)
        assert hg_x * (pow(x, n, r) - 1) % r == c.expression_of(x, values, z_next, permutation=False)


# ---------------------------------------------------------------- refusals on a real context
@pytest.mark.parametrize("curve", CURVES)
def test_overlap_is_refused_and_nothing_is_written(Q, ctx_of, shared, curve):
    import snark_verifier_amd as sv

    r, ctx, k, e = QU.FIELD[curve], ctx_of(curve), 5, 2
    n, n_ext, s = 1 << k, 1 << (k + e), QU.zeta(curve)
    src = _pack(shared[curve][:3 * n_ext])
    d_p, d_o = _dev(src), _fresh(4 * n_ext)  # three extended columns (or coefficient columns); work and h
    _sync()
    p, o = d_p.data_ptr(), d_o.data_ptr()
    prog = (QU.pack_program(Q, [(QU.MUL, 0, Q.COL(0), Q.COL(2, 1), 0)]), [])
    refused = [
        lambda: Q.eval_dev(ctx, p, k, e, 3, prog, p + 32 * n_ext),  # out inside cols
        lambda: Q.eval_dev(ctx, p, k, e, 3, prog, p),
        lambda: Q.eval_dev(ctx, p, k, e, 3, prog, p + 32 * 3 * n_ext - 32),  # a partial overlap, at the end
        lambda: Q.eval_dev(ctx, p + 32, k, e, 3, prog, p),  # ... and at the start
        lambda: Q.extend_dev(ctx, p, k, e, 3, s, p + 32 * 3 * n - 32),
        lambda: Q.div_vanishing_dev(ctx, p, k, e, s, p + 32),
        lambda: Q.quotient_dev(ctx, p, k, e, 3, prog, s, pow(s, -1, r), o, o + 32 * n_ext),  # h inside work
        lambda: Q.quotient_dev(ctx, p, k, e, 3, prog, s, pow(s, -1, r), o, o + 32 * 3 * n_ext - 32),
        lambda: Q.quotient_dev(ctx, p, k, e, 3, prog, s, pow(s, -1, r), o, p + 32 * 3 * n - 32),  # h on the coefficients
        lambda: Q.quotient_dev(ctx, p, k, e, 3, prog, s, pow(s, -1, r), p + 32 * n, o),  # work on the coefficients
    ]
    for i, call in enumerate(refused):
        with pytest.raises(sv.SnarkvError) as err:
            call()
        assert err.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(err.value), i
    ctx.sync()
    assert _bytes(d_p) == src and _bytes(d_o) == b"\xaa" * (32 * 4 * n_ext + GUARD)
    # the context stays usable: the last refused call with its buffers apart
    Q.quotient_dev(ctx, p, k, e, 3, prog, s, pow(s, -1, r), o, o + 32 * 3 * n_ext)
    ctx.sync()
    coeffs = [shared[curve][j * n:(j + 1) * n] for j in range(3)]
    want = QU.quotient(curve, coeffs, k, e, QU.decode(prog[0]), [], s)
    assert _bytes(d_o)[32 * 3 * n_ext:] == _pack(want) + b"\xaa" * GUARD
