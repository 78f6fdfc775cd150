"""Shared helpers of the coset-at-a-time quotient tests (include/snarkv_quotient_cosets.h): the route on Python integers --
the values of a column on the coset (s W^j) H by one size-k transform, the gate program of tests/quotient_util.py run there
with e = 0, the size-k inverse transforms and the join across the cosets -- and the inputs the CPU, host and GPU tests share."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quotient_util as QU  # noqa: E402

U = QU.U
# every (k, e) in 0..4 x 0..3, and e = 8 with n = 2 and n = 4
MODEL_SHAPES = [(k, e) for k in range(5) for e in range(4)] + [(1, 8), (2, 8)]


def coset_shifts(curve, k, e, shift):
    """s W^j for j < 2^e"""
    r, w_ext = QU.FIELD[curve], U.omega(curve, k + e)
    return [shift * pow(w_ext, j, r) % r for j in range(1 << e)]


def coset_values(curve, coeffs, k, e, shift, j):
    """f((s W^j) w^m) for m < n: rows j, j + 2^e, ... of QU.extend"""
    assert len(coeffs) == 1 << k
    return U.reference(curve, list(coeffs), U.FORWARD, coset_shifts(curve, k, e, shift)[j])


def interleave(rows):
    """[j][m] -> the order of the extended coset, i = j + 2^e m"""
    return [rows[i % len(rows)][i // len(rows)] for i in range(len(rows) * len(rows[0]))]


def join(curve, rows, k, e, shift_inv, factors=None):
    """the header's formula: rows[j][t] = coefficient t of the size-k inverse transform of coset j's values ->
    out[t + q n] = s^-(t + q n) 2^-e sum_j W^(-j (t + q n)) g_j rows[j][t]"""
    r, n, n_ext = QU.FIELD[curve], 1 << k, 1 << (k + e)
    w_inv = pow(U.omega(curve, k + e), -1, r)
    g = factors if factors is not None else [1] * (1 << e)
    scale = pow(1 << e, -1, r)
    wp = [1] * n_ext  # W^-x
    for x in range(1, n_ext):
        wp[x] = wp[x - 1] * w_inv % r
    out, sp = [], 1  # s^-T
    for T in range(n_ext):
        t = T % n
        acc = sum(wp[j * T % n_ext] * g[j] % r * rows[j][t] for j in range(1 << e)) % r
        out.append(sp * scale % r * acc % r)
        sp = sp * shift_inv % r
    return out


def join_values(curve, rows, k, e, shift_inv, factors=None):
    """what snarkv_poly_cosets_join_dev computes after the size-k inverse transforms: rows[j][m] are values"""
    return join(curve, [U.reference(curve, list(v), U.INVERSE) for v in rows], k, e, shift_inv, factors)


def quotient_by_cosets(curve, coeff_cols, k, e, instrs, consts, shift):
    """what snarkv_quotient_cosets_dev computes -> the 2^(k+e) coefficients of h"""
    r = QU.FIELD[curve]
    inv = [pow(t, -1, r) if t else 0 for t in QU.vanishing_table(curve, k, e, shift)]  # the zero rule: zero stays zero
    rows = []
    for j in range(1 << e):
        cols = [coset_values(curve, c, k, e, shift, j) for c in coeff_cols]
        rows.append(QU.interpret(curve, cols, k, 0, instrs, consts))
    return join_values(curve, rows, k, e, pow(shift, -1, r), inv)


def root_shift(curve, k, e):
    """a shift with s^n a 2^e-th root of unity other than for s = 1: W itself, for which coset 2^e - 1 vanishes"""
    return U.omega(curve, k + e)


def circuit_columns(curve, k):
    """the 11 coefficient columns of the small circuit at k >= 1 (its Z on integers), random columns below"""
    r = QU.FIELD[curve]
    if k >= 1:
        c = QU.Circuit(curve, k)
        return c.coeff_columns(c.z()[0])
    rnd = random.Random("quotient-cosets-columns-%s-%d" % (curve, k))
    return [[rnd.randrange(r) for _ in range(1 << k)] for _ in range(QU.COLS)]
