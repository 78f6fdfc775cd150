"""CPU: the friendly-multiple products of csrc/fq29.h (fq29_mul_fm / fq29_sqr_fm / fq29_mul2_fm) and the fast adders of
csrc/g1_29.h on them, for BN254 and pallas, against exact integers (tests/fq29_fm_model.py): the g++ build of
tests/hosttest/hosttest_curve_fm.cpp.

  * products: residue, limb shape, the range a*b/2^261 + [0, (1 + 2^-29) p) and the nine limbs of the column model, on the
    operand classes of tests/fq29_model.py (random, the edges of the lazy sets, all-ones limbs) and on 0, 1, p - 1;
  * the column accumulator at the widest operands;
  * the interval argument of the fast adders redone with the wider product range: S closes from S x affine and from
    (S u SJ)^2, on both curves;
  * the `_fm` adders on every corner of S and SJ: the model's limbs, the set again, and the SAME POINT as the pinned adders;
  * a chain of 200 `_fm` mixed additions onto one accumulator: inside S after every step, the oracle's point at the end;
  * the generated bodies and constants are what their generators produce."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fq29_fm_model as FM  # noqa: E402

M = FM.M
CURVE_NAMES = ["bn254", "pallas"]
N = 6000  # records per operand class: the pools put their corners and edge values first


def _special_rows(F):
    q = F.q
    ones = M.land([M.MASK] * 8, 0, 1, F)  # all-ones limbs 0..7, limb 8 as a value inside (-8p, 8p) makes it
    sp = [M.spell(v) for v in (0, 1, q - 1, q, F.one)] + [ones, M.land([M.MASK] * 8, 8 * q, -1, F)]
    return [a + b for a in sp for b in sp]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fm_products_against_exact_integers(curve):
    C = M.CURVES[curve]
    F = C.fq
    run = FM.host_runner(curve)
    cases = M.field_cases(C, N)
    mul = np.concatenate([np.array(_special_rows(F), dtype=np.int32), cases["fq29_mul"]])
    sqr = np.concatenate([mul[:49, :9], cases["fq29_sqr"]])
    sp = mul[:49]
    mul2 = np.concatenate([np.concatenate([sp, -sp[::-1]], axis=1), cases["fq29_mul2"]])
    worst = {}
    for name, inp, npairs in (("fq29_mul_fm", mul, 1), ("fq29_sqr_fm", sqr, 0), ("fq29_mul2_fm", mul2, 2)):
        out = run(name, inp)
        if npairs == 0:
            t = M.vals(inp) ** 2
        else:
            t = sum(M.vals(inp[:, 18 * j:18 * j + 9]) * M.vals(inp[:, 18 * j + 9:18 * j + 18]) for j in range(npairs))
        worst[name] = FM.check_product_fm(F, out, t, "%s %s" % (curve, name))
        for i, r in enumerate(inp.tolist()):  # the column loop itself, with its accumulator watched
            pairs = [(r, r)] if npairs == 0 else [(r[18 * j:18 * j + 9], r[18 * j + 9:18 * j + 18]) for j in range(npairs)]
            lim, _ = FM.mul_columns_fm(F, pairs)
            assert lim == out[i].tolist(), "%s %s: column model differs at %d" % (curve, name, i)
        assert len(out) >= N
    print("largest (out 2^261 - ab) / (p 2^261):", {k: "%.6f" % v for k, v in worst.items()})


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fm_column_accumulator_at_the_widest_operands(curve):
    """one operand at 2^29 - 1, the other at +-2^30.6 in every limb 0..7, and fq29_mul2_fm with all four at +-(2^29 - 1):
    every column of the model (and hence of the C it mirrors line by line) stays inside int64"""
    F = M.CURVES[curve].fq
    run = FM.host_runner(curve)
    peak = 0
    for sa in (1, -1):
        for sb in (1, -1):
            for alt in (0, 1):
                a = M.land([sa * M.MASK * (-1) ** (alt * i) for i in range(8)], 0, 1, F)
                b = M.land([sb * M.W306] * 8, 0, 1, F)
                assert FM.budget_ok_fm(F, [(a, b)])
                lim, pk = FM.mul_columns_fm(F, [(a, b)])
                peak = max(peak, pk)
                assert run("fq29_mul_fm", np.array([a + b], dtype=np.int32)).tolist()[0] == lim
                c = M.land([sb * M.MASK] * 8, 0, 1, F)
                assert FM.budget_ok_fm(F, [(a, c), (c, a)])
                lim, pk = FM.mul_columns_fm(F, [(a, c), (c, a)])
                peak = max(peak, pk)
                assert run("fq29_mul2_fm", np.array([a + c + c + a], dtype=np.int32)).tolist()[0] == lim
    print("peak |acc| = 2^%.2f" % np.log2(float(peak)))
    assert peak < 1 << 63


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_interval_argument_of_the_fast_adders_closes(curve):
    res, seen = FM.interval_closure(M.CURVES[curve])
    assert set(res) == {"madd", "add S+S", "add S+SJ", "add SJ+S", "add SJ+SJ"} and len(seen) == 9 + 4 * 13
    for k, r in res.items():
        print("%-10s x %r  y %r  zz %r  zzz %r" % (k, r.x, r.y, r.zz, r.zzz))


def _point_rows(C, run, op_fm, op_pinned, rows, meta, model, nrec=4):
    """`op_fm` over the rows: the model's limbs, S again, and the point `op_pinned` gives (and the oracle)"""
    out = run(op_fm, M._arr(rows)).tolist()
    ref = run(op_pinned, M._arr(rows)).tolist()
    for i, (row_out, row_ref, (a, pa, b, pb)) in enumerate(zip(out, ref, meta)):
        got, pin = M.unflat(row_out, nrec), M.unflat(row_ref, nrec)
        what = "%s %s #%d" % (C.name, op_fm, i)
        assert got == model(a, b), what + ": limbs differ from the model"
        bad = M.in_closed_set(C, got)
        assert bad is None, what + ": " + bad
        assert M.point_of_xyzz(C, got) == M.point_of_xyzz(C, pin) == C.O.g1_add(pa, pb), what + ": not the pinned adder's point"
        # (the limbs are almost always the pinned ones too: the two representatives differ only when the pinned digits m
        # are below 2^232, where the `_fm` product returns that value + p)
    return len(rows)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_fm_adders_are_the_pinned_adders_as_points(curve):
    C = M.CURVES[curve]
    F = C.fq
    run = FM.host_runner(curve)
    rnd = random.Random(61)
    S = M.corner_accs(C, 600, 21)
    SJ = M.corner_accs(C, 200, 22, chain=True)
    aff = [(M.affine_rec(C, p), p) for p in M.base_points(C, 48)]
    rows, meta = [], []
    for rec, pt in S:
        for neg in (False, True):  # an entry's sign bit negates y limb-wise
            b, pb = M._other(rnd, aff, pt, C)
            if neg:
                b, pb = [b[0], M.l_neg(b[1])], C.O.g1_neg(pb)
            rows.append(M.flat(rec, b))
            meta.append((rec, pt, b, pb))
    n = _point_rows(C, run, "xyzz29_madd_fast_fm", "xyzz29_madd_fast", rows, meta, lambda a, b: FM.m_madd_fast_fm(F, a, b))
    assert n >= 1200
    rows, meta = [], []
    both = S + SJ
    for rec, pt in both:
        for _ in range(2):
            b, pb = M._other(rnd, both, pt, C)
            rows.append(M.flat(rec, b))
            meta.append((rec, pt, b, pb))
    n = _point_rows(C, run, "xyzz29_add_fast_fm", "xyzz29_add_fast", rows, meta, lambda a, b: FM.m_add_fast_fm(F, a, b))
    assert n >= 1600
    sk = run("xyzz29_add_skipid_fast_fm", M._arr([r + [0] for r in rows]))
    assert (sk[:, 36] == 0).all() and (sk[:, :36] == run("xyzz29_add_fast_fm", M._arr(rows))).all()
    # the stored identity on either side: the other operand, untouched
    ident = [[0] * 9] * 4
    rec = S[0][0]
    sk = run("xyzz29_add_skipid_fast_fm", M._arr([M.flat(rec, ident) + [0], M.flat(ident, rec) + [0]])).tolist()
    assert sk[0][:36] == M.flat(rec) and sk[1][:36] == M.flat(rec) and sk[0][36] == sk[1][36] == 0


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_chain_of_200_fm_mixed_additions_stays_inside_the_set(curve):
    C = M.CURVES[curve]
    F, O = C.fq, C.O
    run = FM.host_runner(curve)
    rnd = random.Random(67)
    pts = M.base_points(C, 48)
    for start in (0, 7, 30):  # three corners of S to start from
        rec, pt = M.corner_accs(C, 600, 21)[start]
        rows, want, model = [], pt, rec
        for i in range(200):
            q = pts[(start + 1 + i) % 48]  # repeated points are fine: the running sum is never +-one of them
            a = M.affine_rec(C, q)
            if rnd.random() < 0.5:
                a, q = [a[0], M.l_neg(a[1])], O.g1_neg(q)
            rows.append(M.flat(rec if i == 0 else [[0] * 9] * 4, a))
            want = O.g1_add(want, q)
            model = FM.m_madd_fast_fm(F, model, a)  # asserts the limb budget before each of its ten products
        out = run("madd_chain_fm", M._arr(rows)).tolist()
        for i, row in enumerate(out):
            bad = M.in_closed_set(C, M.unflat(row, 4))
            assert bad is None, "%s step %d: %s" % (curve, i, bad)
        assert M.unflat(out[-1], 4) == model and M.point_of_xyzz(C, model) == want


def test_generated_fm_sources_are_current():
    csrc = os.path.join(M.ROOT, "snark-verifier_amd", "csrc")
    for kind in ("mul_fm", "mul2_fm", "sqr_fm"):
        out = subprocess.run([sys.executable, os.path.join(csrc, "gen_fq29_mul_asm.py"), kind], check=True, capture_output=True,
                             text=True).stdout
        assert out == open(os.path.join(csrc, "fq29_%s_asm.inc" % kind)).read(), kind
        assert "v_mad_i64_i32" in out and out.count("SNARKV_FQ29_NINV") == 2 * 2, kind  # digits 7 and 8 only, both curves
    for curve, header in (("bn254", "bn254_consts.h"), ("pallas", "pallas_consts.h")):
        txt = open(os.path.join(csrc, header)).read()
        line = next(l for l in txt.split("\n") if l.startswith("#define SNARKV_FQ29_FM_LIMBS"))
        limbs = [int(x, 16) for x in line[line.index("{") + 1:line.index("}")].split(",")]
        assert limbs == FM.fm_limbs(M.CURVES[curve].fq) and limbs[0] == M.MASK, curve
