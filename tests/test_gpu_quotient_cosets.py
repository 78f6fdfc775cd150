"""GPU: the coset-at-a-time quotient (snark_verifier_amd.quotient.cosets_dev and cosets_join_dev,
include/snarkv_quotient_cosets.h) on BN254 and pallas, byte for byte on canonical words against quotient_dev and against
Python integers (tests/quotient_util.py): from one row to the coset transform past its one-tile path (k = 10), e = 0 (the
join is a scaling) to e = 8 (256 cosets of 2 and of 4 rows, n smaller than the join's tile), rotations -512 and 511 that wrap
many times within a coset, the shift 1 (a vanishing entry is zero), one column, a broken witness, the way back on its own in
place and out of place against the large inverse transform, and two calls back to back with different shapes on one context.

Nothing is filtered: every output buffer starts as 0xAA bytes with a guard behind it, and the whole of it is compared.  The
work buffer has exactly n_cols * n elements and its guard is checked; the coefficient columns are compared afterwards."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quotient_cosets_util as CU  # noqa: E402
import quotient_util as QU  # noqa: E402

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "pallas"]
# (8, 1) | (8, 2): k + e on the two sides of the large transform's one-tile path; (10, 2): the coset transform past it;
# (1, 8), (2, 8): n below the join's tile of four t; (9, 3): two tiles of 128 t
SHAPES = [(0, 0), (0, 3), (1, 1), (3, 2), (8, 1), (8, 2), (7, 3), (1, 8), (2, 8), (10, 2), (9, 3)]
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


_CASES = {}


def _case(Q, curve, k, e):
    """the 11 coefficient columns, a 64-instruction random program over the rotations -512, -1, 0, 1, 511, its constants and
    the integers' h at the shift zeta -- computed once per shape, never changed"""
    if (curve, k, e) not in _CASES:
        r = QU.FIELD[curve]
        rnd = random.Random("gpu-quotient-cosets-%s-%d-%d" % (curve, k, e))
        coeffs = CU.circuit_columns(curve, k)
        instrs = QU.random_program(Q, rnd, 64, QU.COLS, 5)
        assert {QU.ROTATIONS[0], QU.ROTATIONS[-1]} <= {((w >> 20) & 0x3FF) - (1024 if (w >> 20) & 0x200 else 0)
                                                       for i in instrs for w in i[2:] if w >> 30 == 2}
        consts = [rnd.randrange(r) for _ in range(5)]
        want = QU.quotient(curve, coeffs, k, e, instrs, consts, QU.zeta(curve))
        _CASES[(curve, k, e)] = (coeffs, instrs, consts, want)
    return _CASES[(curve, k, e)]


def _both_routes(Q, ctx, curve, coeffs, k, e, prog, s):
    """quotient_dev and cosets_dev over the same columns -> the bytes of h both wrote (asserted equal, guards and inputs
    checked)"""
    r, n, n_ext, n_cols = QU.FIELD[curve], 1 << k, 1 << (k + e), len(coeffs)
    s_inv = pow(s, -1, r)
    src = _pack(sum(coeffs, []))
    d_coeffs = _dev(src)
    d_work_q, d_h_q = _fresh(n_cols * n_ext), _fresh(n_ext)
    d_work_c, d_h_c = _fresh(n_cols * n), _fresh(n_ext)  # exactly n_cols * n elements
    _sync()
    Q.quotient_dev(ctx, d_coeffs, k, e, n_cols, prog, s, s_inv, d_work_q, d_h_q)
    Q.cosets_dev(ctx, d_coeffs, k, e, n_cols, prog, s, s_inv, d_work_c, d_h_c)
    ctx.sync()
    got_q, got_c = _bytes(d_h_q), _bytes(d_h_c)
    assert got_c == got_q and got_c[32 * n_ext:] == b"\xaa" * GUARD
    assert _bytes(d_work_c)[32 * n_cols * n:] == b"\xaa" * GUARD and _bytes(d_coeffs) == src
    return got_c[:32 * n_ext]


@pytest.mark.parametrize("k,e", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_cosets_against_quotient_dev_and_the_integers(Q, ctx_of, curve, k, e):
    coeffs, instrs, consts, want = _case(Q, curve, k, e)
    got = _both_routes(Q, ctx_of(curve), curve, coeffs, k, e, (QU.pack_program(Q, instrs), consts), QU.zeta(curve))
    assert got == _pack(want)


@pytest.mark.parametrize("curve", CURVES)
def test_rotations_that_wrap_many_times_within_a_coset(Q, ctx_of, curve):
    """n = 8: -512 and 511 rows of the coset wrap 64 times"""
    r, k, e = QU.FIELD[curve], 3, 2
    rnd = random.Random("gpu-quotient-cosets-wrap-" + curve)
    coeffs = [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(2)]
    instrs = [(QU.MUL, 1, Q.COL(0, -512), Q.COL(1, 511), 0), (QU.ADD, 2, Q.COL(1, -512), Q.COL(0, 511), 0),
              (QU.FMA, 0, Q.REG(1), Q.COL(0, 3), Q.REG(2)), (QU.SUB, 0, Q.REG(0), Q.COL(1, -5), 0)]
    got = _both_routes(Q, ctx_of(curve), curve, coeffs, k, e, (QU.pack_program(Q, instrs), []), QU.zeta(curve))
    assert got == _pack(QU.quotient(curve, coeffs, k, e, instrs, [], QU.zeta(curve)))


@pytest.mark.parametrize("shift", ["one", "W"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_zero_rule(Q, ctx_of, curve, shift):
    """s^n a 2^e-th root of unity: a vanishing entry is zero and stays zero (entry 0 for s = 1, the last for s = W); the rows of
    that coset count as zero on both routes"""
    k, e = 3, 2
    coeffs, instrs, consts, _ = _case(Q, curve, k, e)
    s = 1 if shift == "one" else CU.root_shift(curve, k, e)
    assert QU.vanishing_table(curve, k, e, s)[0 if shift == "one" else -1] == 0
    got = _both_routes(Q, ctx_of(curve), curve, coeffs, k, e, (QU.pack_program(Q, instrs), consts), s)
    assert got == _pack(QU.quotient(curve, coeffs, k, e, instrs, consts, s))


@pytest.mark.parametrize("curve", CURVES)
def test_one_column(Q, ctx_of, curve):
    r, k, e = QU.FIELD[curve], 5, 2
    rnd = random.Random("gpu-quotient-cosets-one-column-" + curve)
    coeffs = [[rnd.randrange(r) for _ in range(1 << k)]]
    instrs = QU.random_program(Q, rnd, 24, 1, 2)
    consts = [rnd.randrange(r) for _ in range(2)]
    got = _both_routes(Q, ctx_of(curve), curve, coeffs, k, e, (QU.pack_program(Q, instrs), consts), QU.zeta(curve))
    assert got == _pack(QU.quotient(curve, coeffs, k, e, instrs, consts, QU.zeta(curve)))


@pytest.mark.parametrize("bad", [None, "gate", "copy"])
@pytest.mark.parametrize("curve", CURVES)
def test_the_small_circuit_and_a_broken_witness(Q, ctx_of, curve, bad):
    """the circuit's own program at k = 4, e = 2: a good witness leaves the coefficients from 3n - 3 on zero, a broken one
    gives an h that is no polynomial multiple -- and both routes still write the same bytes"""
    k, e = 4, 2
    c = QU.Circuit(curve, k, bad)
    coeffs = c.coeff_columns(c.z()[0])
    p = c.program(Q)
    got = _both_routes(Q, ctx_of(curve), curve, coeffs, k, e, p, QU.zeta(curve))
    h = QU.quotient(curve, coeffs, k, e, p.instrs, p.consts, QU.zeta(curve))
    assert got == _pack(h)
    assert all(v == 0 for v in h[3 * (1 << k) - 3:]) == (bad is None)


@pytest.mark.parametrize("k,e", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_the_join_against_the_large_inverse_transform(Q, ctx_of, curve, k, e):
    from snark_verifier_amd import ntt

    r, ctx, s = QU.FIELD[curve], ctx_of(curve), QU.zeta(curve)
    s_inv = pow(s, -1, r)
    n, n_ext = 1 << k, 1 << (k + e)
    rnd = random.Random("gpu-quotient-cosets-join-%s-%d-%d" % (curve, k, e))
    rows = [[rnd.randrange(r) for _ in range(n)] for _ in range(1 << e)]
    src = _pack(sum(rows, []))
    d_in, d_out, d_big = _dev(src), _fresh(n_ext), _dev(_pack(CU.interleave(rows)))
    _sync()
    Q.cosets_join_dev(ctx, d_in, k, e, s_inv, d_out)
    ntt.intt_dev(ctx, d_big, d_big, k + e, 1, shift=s_inv)
    ctx.sync()
    got = _bytes(d_out)
    assert got == _bytes(d_big) + b"\xaa" * GUARD and _bytes(d_in) == src
    assert got[:32 * n_ext] == _pack(QU.to_coeffs(curve, CU.interleave(rows), s_inv))
    d_same = _dev(src + b"\xaa" * GUARD)
    _sync()
    Q.cosets_join_dev(ctx, d_same, k, e, s_inv, d_same)  # in place: the same bytes
    ctx.sync()
    assert _bytes(d_same) == got


@pytest.mark.parametrize("curve", CURVES)
def test_two_calls_back_to_back_with_different_shapes(Q, ctx_of, curve):
    """one context, no synchronisation between the calls: the transform's tables of w are refilled for the other k, the
    quotient's slot is staged again behind the first call's join"""
    ctx, s = ctx_of(curve), QU.zeta(curve)
    s_inv = pow(s, -1, QU.FIELD[curve])
    runs = []
    for k, e in ((8, 2), (3, 2), (7, 3)):
        coeffs, instrs, consts, want = _case(Q, curve, k, e)
        n = 1 << k
        runs.append((_dev(_pack(sum(coeffs, []))), _fresh(QU.COLS * n), _fresh(n << e), k, e, (QU.pack_program(Q, instrs), consts), want))
    _sync()
    for d_coeffs, d_work, d_h, k, e, prog, _ in runs:
        Q.cosets_dev(ctx, d_coeffs, k, e, QU.COLS, prog, s, s_inv, d_work, d_h)
    ctx.sync()
    for _, d_work, d_h, k, e, _, want in runs:
        assert _bytes(d_h) == _pack(want) + b"\xaa" * GUARD, (k, e)
        assert _bytes(d_work)[32 * QU.COLS << k:] == b"\xaa" * GUARD


@pytest.mark.parametrize("curve", CURVES)
def test_overlap_is_refused_and_nothing_is_written(Q, ctx_of, curve):
    import snark_verifier_amd as sv

    r, ctx, k, e = QU.FIELD[curve], ctx_of(curve), 5, 2
    n, n_ext, s = 1 << k, 1 << (k + e), QU.zeta(curve)
    s_inv = pow(s, -1, r)
    rnd = random.Random("gpu-quotient-cosets-overlap-" + curve)
    coeffs = [[rnd.randrange(r) for _ in range(n)] for _ in range(3)]
    src = _pack(sum(coeffs, []))
    d_p, d_o = _dev(src), _fresh(3 * n + n_ext)  # work (3 n) and h (N), back to back
    _sync()
    p, o = d_p.data_ptr(), d_o.data_ptr()
    instrs = [(QU.MUL, 0, Q.COL(0), Q.COL(2, 1), 0)]
    prog = (QU.pack_program(Q, instrs), [])
    refused = [
        lambda: Q.cosets_dev(ctx, p, k, e, 3, prog, s, s_inv, o, o + 32 * 3 * n - 32),  # h on the last element of work
        lambda: Q.cosets_dev(ctx, p, k, e, 3, prog, s, s_inv, o, o),
        lambda: Q.cosets_dev(ctx, p, k, e, 3, prog, s, s_inv, o, p + 32 * 3 * n - 32),  # h on the coefficients
        lambda: Q.cosets_dev(ctx, p, k, e, 3, prog, s, s_inv, p + 32 * n, o),  # work on the coefficients
        lambda: Q.cosets_join_dev(ctx, o, k, e, s_inv, o + 32),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(sv.SnarkvError) as err:
            call()
        assert err.value.code == sv.SNARKV_ERR_ARG and "overlap" in str(err.value), i
    ctx.sync()
    assert _bytes(d_p) == src and _bytes(d_o) == b"\xaa" * (32 * (3 * n + n_ext) + GUARD)
    # the context stays usable: h right behind a work buffer of 3 n elements
    Q.cosets_dev(ctx, p, k, e, 3, prog, s, s_inv, o, o + 32 * 3 * n)
    ctx.sync()
    want = QU.quotient(curve, coeffs, k, e, instrs, [], s)
    assert _bytes(d_o)[32 * 3 * n:] == _pack(want) + b"\xaa" * GUARD and _bytes(d_p) == src
