"""Exact-integer model of the friendly-multiple products of csrc/fq29.h (fq29_mul_fm / fq29_sqr_fm / fq29_mul2_fm) and of the
fast adders of csrc/g1_29.h run on them, on top of tests/fq29_model.py (imported, not edited).

The product.  M = NINV * p has limb 0 = 2^29 - 1.  Reduction step k < FM_STEPS takes the digit q = (column k) & (2^29 - 1)
and adds q M 2^(29 k): column k needs no product (acc + q (2^29 - 1) has its low 29 bits clear and carries (acc >> 29) + q),
the + q rides in limb 1 of the constant.  Steps 7 and 8 are the ordinary ones (digit by NINV, multiple of p).  What is added
is a multiple of p, so the residue is that of a*b/2^261; it is below 2^203 M + 2^261 p <= (2^-29 + 1) p 2^261, so
    out  in  a*b/2^261 + [0, (1 + 2^-29) p)
against [0, p) of the pinned products.  There is no closed form of the nine limbs other than the column loop itself:
`mul_columns_fm` is the reference for raw limbs.

The interval argument.  `interval_closure` runs the TEXT of xyzz29_madd_fast / xyzz29_add_fast / xyzz29_finish (read from
g1_29.h by fq29_model's translator) on intervals in units of p, a product being  [min uv, max uv] / (2^261 / p) + [0, 1 + 2^-29)
rounded outward, and requires the accumulator set S of the header again -- from S x affine for the mixed adder and from
(S u SJ)^2 for the full one."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fq29_model as M  # noqa: E402

MASK = M.MASK
FM_STEPS = 7  # kFq29FmSteps

# name -> (words in, words out): the table of tests/hosttest/hosttest_curve_fm.cpp
OPS = {"fq29_mul_fm": (18, 9), "fq29_sqr_fm": (9, 9), "fq29_mul2_fm": (36, 9), "xyzz29_madd_fast_fm": (54, 36),
       "xyzz29_add_fast_fm": (72, 36), "xyzz29_add_skipid_fast_fm": (73, 37), "madd_chain_fm": (54, 36),
       "xyzz29_madd_fast": (54, 36), "xyzz29_add_fast": (72, 36)}


def fm_limbs(F):
    """the ten limbs of M = NINV p, limb 1 incremented (SNARKV_FQ29_FM_LIMBS)"""
    m = F.ninv * F.q
    l = [(m >> (29 * i)) & MASK for i in range(10)]
    assert l[0] == MASK and m >> 290 == 0
    l[1] += 1
    return l


def mul_columns_fm(F, pairs):
    """the column loop of fq29_mul_fm / fq29_mul2_fm / fq29_sqr_fm (plain-C form) on Python integers.
    Returns (limbs, peak |acc|); asserts that int64 never wraps."""
    m, r, acc, peak = [0] * 9, [0] * 9, 0, 0
    p, fm = F.limbs, fm_limbs(F)

    def see(x):
        nonlocal peak
        peak = max(peak, abs(x))
        assert -(1 << 63) <= x < (1 << 63), "column accumulator left int64"
        return x

    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        for a, b in pairs:
            for i in range(lo, hi + 1):
                acc = see(acc + a[i] * b[k - i])
        for i in range(min(k, 9)):
            j = k - i
            if i < FM_STEPS:
                if j <= 9:
                    acc = see(acc + m[i] * fm[j])
            elif j <= 8:
                acc = see(acc + m[i] * p[j])
        if k < FM_STEPS:
            m[k] = acc & MASK
        elif k < 9:
            m[k] = ((acc & 0xFFFFFFFF) * F.ninv) & MASK
            acc = see(acc + m[k] * p[0])
            assert acc & MASK == 0
        else:
            r[k - 9] = acc & MASK
        acc >>= 29
    r[8] = M._i32(acc)
    return r, peak


def budget_ok_fm(F, pairs):
    """exact per-column bound: operand products + (2^29 - 1) * (the constants of the column) + carry below 2^63"""
    p, fm = F.limbs, fm_limbs(F)
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        s = sum(abs(a[i]) * abs(b[k - i]) for a, b in pairs for i in range(lo, hi + 1))
        red = sum(fm[k - i] for i in range(min(k, FM_STEPS)) if k - i <= 9)
        red += sum(p[k - i] for i in range(FM_STEPS, min(k + 1, 9)) if k - i <= 8)
        if s + MASK * red + (1 << 35) >= 1 << 63:
            return False
    return True


def m_mul_fm(F, a, b):
    assert M._maxabs(a) * M._maxabs(b) <= 2 ** 59.6, "product outside its operand classes"
    assert budget_ok_fm(F, [(a, b)]), "product outside the column budget"
    return mul_columns_fm(F, [(a, b)])[0]


def m_sqr_fm(F, a):
    assert M._maxabs(a) < 1 << 29, "fq29_sqr_fm needs |limb| < 2^29"
    return mul_columns_fm(F, [(a, a)])[0]


def m_mul2_fm(F, a, b, c, d):
    for x in (a, b, c, d):
        assert M._maxabs(x) < 1 << 29, "fq29_mul2_fm needs |limb| < 2^29 on all four operands"
    return mul_columns_fm(F, [(a, b), (c, d)])[0]


def check_product_fm(F, out, t, what):
    """residue, shape and range of `_fm` product outputs: `out` (n, 9) int32, `t` the exact integers sum a*b"""
    out = np.asarray(out)
    assert out.shape == (len(t), 9), what
    assert ((out[:, :8] >= 0) & (out[:, :8] <= MASK)).all(), what + ": a limb 0..7 outside [0, 2^29)"
    assert (np.abs(out[:, 8].astype(np.int64)) < (1 << 26)).all(), what + ": limb 8 too large"
    d = M.vals(out) * F.R - t
    bad = [i for i, x in enumerate(d) if x % F.q != 0]
    assert not bad, "%s: residue wrong at %d elements, first %d" % (what, len(bad), bad[0])
    top = F.q * F.R + (F.q * F.R >> 29)
    bad = [i for i, x in enumerate(d) if not 0 <= x < top]
    assert not bad, "%s: value outside a*b/2^261 + [0, (1 + 2^-29) q) at %d elements, first %d" % (what, len(bad), bad[0])
    return max(d) / (F.q * F.R)


_CACHE = {}


def formulas_fm(F):
    """the straight-line formulas of g1_29.h executed on limb lists with the `_fm` model products"""
    key = (F.q, "fm")
    if key not in _CACHE:
        src = open(os.path.join(M.ROOT, "snark-verifier_amd", "csrc", "g1_29.h")).read()
        env = {"_NS": M._NS, "fq29_mul": lambda a, b: m_mul_fm(F, a, b), "fq29_sqr": lambda a: m_sqr_fm(F, a),
               "fq29_mul2": lambda a, b, c, d: m_mul2_fm(F, a, b, c, d), "fq29_norm": M.l_norm, "fq29_sub": M.l_sub,
               "fq29_add": M.l_add, "fq29_dbl": M.l_dbl, "fq29_neg": M.l_neg}
        for name in ("xyzz29_finish", "xyzz29_madd_fast", "xyzz29_add_fast"):
            exec(M._translate(src, name), env)
        _CACHE[key] = env
    return _CACHE[key]


def m_madd_fast_fm(F, acc, p):
    a, b = M._NS(acc), M._NS()
    b.x, b.y = p
    return formulas_fm(F)["xyzz29_madd_fast"](a, b).rec()


def m_add_fast_fm(F, acc, b):
    return formulas_fm(F)["xyzz29_add_fast"](M._NS(acc), M._NS(b)).rec()


# ---------------------------------------------------------------- the interval argument
class Iv:
    """closed interval [lo, hi] in units of p, exact rationals"""

    def __init__(self, lo, hi):
        self.lo, self.hi = Fraction(lo), Fraction(hi)
        assert self.lo <= self.hi

    def within(self, lo, hi):
        return lo < self.lo and self.hi < hi

    def __repr__(self):
        return "[%.4f, %.4f]" % (float(self.lo), float(self.hi))


def interval_closure(C):
    """Runs the text of the fast adders on intervals.  Returns {name: Iv} of every product output and of the results;
    asserts that every result is inside S (M.in_closed_set's intervals) again."""
    q = C.fq.q
    rho = Fraction(C.fq.R, q)
    top = 1 + Fraction(1, 1 << 29)
    seen = {}

    def prod(pairs, name):
        lo = hi = Fraction(0)
        for a, b in pairs:
            if a is b:  # a square
                c = [a.lo * a.lo, a.hi * a.hi]
                lo += 0 if a.lo <= 0 <= a.hi else min(c)
                hi += max(c)
            else:
                c = [a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi]
                lo += min(c)
                hi += max(c)
        r = Iv(lo / rho, hi / rho + top)
        k = "%s#%d" % (name, len(seen))
        seen[k] = r
        return r

    env = {"_NS": M._NS, "fq29_mul": lambda a, b: prod([(a, b)], "mul"), "fq29_sqr": lambda a: prod([(a, a)], "sqr"),
           "fq29_mul2": lambda a, b, c, d: prod([(a, b), (c, d)], "mul2"), "fq29_norm": lambda a: a,
           "fq29_sub": lambda a, b: Iv(a.lo - b.hi, a.hi - b.lo), "fq29_add": lambda a, b: Iv(a.lo + b.lo, a.hi + b.hi),
           "fq29_dbl": lambda a: Iv(2 * a.lo, 2 * a.hi), "fq29_neg": lambda a: Iv(-a.hi, -a.lo)}
    src = open(os.path.join(M.ROOT, "snark-verifier_amd", "csrc", "g1_29.h")).read()
    for name in ("xyzz29_finish", "xyzz29_madd_fast", "xyzz29_add_fast"):
        exec(M._translate(src, name), env)
    n_out = Iv(Fraction(-1, 4), Fraction(5, 4))  # a product output as S keeps it (open ends: within() is strict below)

    def s_rec(x=(-4, 2), y=(-2, 2)):
        return M._NS([Iv(*x), Iv(*y), n_out, n_out])

    def in_s(r, what):
        assert r.x.within(-4, 2), "%s %s: x leaves (-4p, 2p): %r" % (C.name, what, r.x)
        assert r.y.within(-2, 2), "%s %s: y leaves (-2p, 2p): %r" % (C.name, what, r.y)
        assert r.zz.within(Fraction(-1, 4), Fraction(5, 4)), "%s %s: zz leaves (-p/4, 5p/4): %r" % (C.name, what, r.zz)
        assert r.zzz.within(Fraction(-1, 4), Fraction(5, 4)), "%s %s: zzz leaves (-p/4, 5p/4): %r" % (C.name, what, r.zzz)

    res = {}
    aff = M._NS()
    aff.x, aff.y = Iv(0, 1), Iv(-1, 1)  # canonical x; y or its limb-wise negation (an entry's sign bit)
    r = env["xyzz29_madd_fast"](s_rec(), aff)
    in_s(r, "madd")
    res["madd"] = r
    sj = dict(x=(-6, 11), y=(Fraction(-19, 2), 2))  # what a Jacobian doubling chain leaves: legal as either operand of add
    for na, a in (("S", {}), ("SJ", sj)):
        for nb, b in (("S", {}), ("SJ", sj)):
            r = env["xyzz29_add_fast"](s_rec(**a), s_rec(**b))
            in_s(r, "add %s + %s" % (na, nb))
            res["add %s+%s" % (na, nb)] = r
    return res, seen


# ---------------------------------------------------------------- the host build
def host_runner(curve):
    """tests/hosttest/hosttest_curve_fm.cpp compiled with g++ (the plain-C bodies): run(op, (n, words in)) -> (n, words out)"""
    import ctypes

    key = ("lib", curve)
    if key not in _CACHE:
        lib = ctypes.CDLL(M.load_build().build_hosttest("curve_fm", curve))
        lib.hf_curve.restype = ctypes.c_char_p
        assert lib.hf_curve() == curve.encode()
        for op, (wi, wo) in OPS.items():
            assert getattr(lib, "hf_%s_io" % op)() == (wi << 16) | wo, op
        _CACHE[key] = lib
    lib = _CACHE[key]

    def run(op, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.ndim == 2 and a.shape[1] == OPS[op][0], op
        out = np.zeros((len(a), OPS[op][1]), dtype=np.int32)
        getattr(lib, "hf_%s" % op)(a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), len(a))
        return out

    return run
