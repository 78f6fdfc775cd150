"""Exact-integer model of the lazy 9 x 29-bit field layer (csrc/fq29.h, fr29.h) and of the XYZZ / Jacobian formulas built on
it (csrc/g1_29.h), the operand generators that sit on the edges of the lazy-value contract, and the checks shared by
tests/test_curve_math_lazy_host.py (g++ build) and tests/test_gpu_field_layer.py (device builds).  Plain module: Python
integers and numpy only, no fixtures.  The `run(op, array) -> array` callable that every check takes feeds raw int32
records to one build of tests/hosttest/curve_ops.h.

The value of a limb record is val(l) = sum l_i 2^(29 i) over the raw signed limbs.

Budget of a product.  fq29.h words it as 9 max|a_i| max|b_j| < 2^63 - 2^61.2 "i.e." max|a_i| max|b_j| < 2^59.6 (one operand
below 2^29, the other up to 2^30.6; or both below 2^29.8).  The two halves disagree: 9 * 2^59.6 = 2^62.77 is above
2^63 - 2^61.2 = 2^62.51.  What the algorithm needs is that no COLUMN of the product scanning loop leaves int64, so that is
what `budget_ok` / `budget_mask` check, exactly and per element: for every column k,
    sum_i |a_i| |b_(k-i)|  +  (2^29 - 1) * sum_j p_j  +  2^35  <  2^63
(the reduction digits are < 2^29, the carry into a column is below 2^34 once the previous column fitted), next to the
operand classes themselves (max|a_i| max|b_j| <= 2^59.6).  Limb 8 of a value within (-8p, 8p) is small, which is why the
widest class fits although 9 * 2^59.6 does not."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

MASK = (1 << 29) - 1
RBITS = 261
W306 = int(2 ** 30.6)   # the widest limb of the wide operand of a product
W298 = int(2 ** 29.8)   # both operands this wide
I32 = 1 << 31

# name -> (words in, words out): the table of tests/hosttest/curve_ops.h
OPS = {
    "fq29_mul": (18, 9), "fq29_sqr": (9, 9), "fq29_mul2": (36, 9), "fq29_norm": (9, 9), "fq29_canon_of_product": (9, 9),
    "fq29_canon_residue": (9, 9), "fq29_is_zero_mod_p": (9, 1), "fq29_from_words": (8, 9), "fq29_from_words_mont": (8, 9),
    "fq29_to_words": (9, 8), "fq29_to_words_mont": (9, 8), "fq29_pack256": (9, 8), "fq29_unpack256": (8, 9),
    "fr29_mul": (18, 9), "fr29_mul2": (36, 9), "fr29_from_canonical": (8, 9), "fr29_to_canonical": (9, 8),
    "fr29_pow5": (9, 9), "fr29_canon_residue": (9, 9), "fq_mul": (16, 8),
    "xyzz29_madd_fast": (54, 36), "xyzz29_add_fast": (72, 36), "xyzz29_madd_careful": (54, 36),
    "xyzz29_add_careful": (72, 36), "xyzz29_add_skipid_fast": (73, 37), "xyzz29_double": (36, 36),
    "jac29_double": (28, 27), "xyzz29_double_n": (37, 36), "jac29_to_xyzz": (27, 36), "xyzz29_is_degenerate": (36, 1),
    "xyzz29_to_affine": (36, 18), "g1_29_scalar_mul_fast": (26, 36), "g1_29_scalar_mul_careful": (26, 36),
    "glv_decompose": (8, 8), "glv_w3_digits": (4, 43),
}


class Field:
    """A 9 x 29 Montgomery field (R = 2^261) with modulus q"""

    def __init__(self, q):
        self.q = q
        self.R = 1 << RBITS
        self.limbs = spell(q)
        self.ninv = (-pow(q, -1, 1 << 29)) % (1 << 29)
        self.nqinv = (-pow(q, -1, self.R)) % self.R
        self.one = self.R % q
        self.rinv = pow(self.R, -1, q)


class Curve:
    def __init__(self, name, O):
        self.name, self.O = name, O
        self.fq, self.fr = Field(O.P), Field(O.R)
        self.b = getattr(O, "B1", 3)


# ---------------------------------------------------------------- limbs <-> integers
def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def vals(a):
    """(n, 9) int32 array -> object array of n Python integers"""
    a = np.asarray(a)
    out = a[:, 0].astype(object)
    for i in range(1, a.shape[1]):
        out = out + (a[:, i].astype(object) << (29 * i))
    return out


def spell(v):
    """carry-normalised limbs of any integer: limbs 0..7 in [0, 2^29), limb 8 the (signed) rest"""
    l = [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]
    assert -I32 <= l[8] < I32
    return l


def words_of(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def int_of_words(w):
    return sum((int(x) & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(w))


def words_i32(v):
    return [x - (1 << 32) if x >= I32 else x for x in words_of(v)]


def _i32(x):
    assert -I32 <= x < I32, "int32 overflow in a limb: %d" % x
    return x


def is_norm(l):
    return all(0 <= x <= MASK for x in l[:8]) and -I32 <= l[8] < I32


def l_add(a, b):
    return [_i32(x + y) for x, y in zip(a, b)]


def l_sub(a, b):
    return [_i32(x - y) for x, y in zip(a, b)]


def l_neg(a):
    return [_i32(-x) for x in a]


def l_dbl(a):
    return [_i32(2 * x) for x in a]


def l_norm(a):
    """fq29_norm, line by line"""
    r, c = [], 0
    for i in range(8):
        t = _i32(a[i] + c)
        r.append(t & MASK)
        c = t >> 29
    r.append(_i32(a[8] + c))
    return r


CURVES = {"bn254": Curve("bn254", BN), "pallas": Curve("pallas", PA)}


# ---------------------------------------------------------------- products
def mul_columns(F, pairs):
    """The product scanning loop of fq29_mul / fq29_mul2 / fq29_sqr (plain-C form), line by line on Python integers:
    sum of a*b over `pairs` with one Montgomery reduction.  Returns (limbs, peak |acc|); asserts int64 never wraps."""
    m, r, acc, peak = [0] * 9, [0] * 9, 0, 0
    p = F.limbs

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
        for i in range(lo, hi + 1):
            if i < k and k - i <= 8:
                acc = see(acc + m[i] * p[k - i])
        if k < 9:
            m[k] = ((acc & 0xFFFFFFFF) * F.ninv) & MASK
            acc = see(acc + m[k] * p[0])
            assert acc & MASK == 0
        else:
            r[k - 9] = acc & MASK
        acc >>= 29
    r[8] = _i32(acc)
    return r, peak


def mul_closed(F, pairs):
    """The same nine limbs in closed form: (sum a b + m q) / 2^261 with m = -(sum a b) / q mod 2^261, carry-normalised"""
    t = sum(val(a) * val(b) for a, b in pairs)
    m = (t * F.nqinv) % F.R
    v = t + m * F.q
    assert v % F.R == 0
    return spell(v >> RBITS)


def _maxabs(l):
    return max(abs(x) for x in l)


def budget_ok(F, a, b):
    """exact per-column bound for ONE product a*b (see the module docstring)"""
    p = F.limbs
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        s = sum(abs(a[i]) * abs(b[k - i]) for i in range(lo, hi + 1))
        red = MASK * sum(p[k - i] for i in range(lo, hi + 1) if k - i <= 8 and i <= k)
        if s + red + (1 << 35) >= 1 << 63:
            return False
    return True


def m_mul(F, a, b):
    """model fq29_mul with its precondition asserted"""
    assert _maxabs(a) * _maxabs(b) <= 2 ** 59.6, "product outside its operand classes"
    assert budget_ok(F, a, b), "product outside the column budget"
    return mul_closed(F, [(a, b)])


def m_sqr(F, a):
    assert _maxabs(a) < 1 << 29, "fq29_sqr needs |limb| < 2^29"
    return mul_closed(F, [(a, a)])


def m_mul2(F, a, b, c, d):
    for x in (a, b, c, d):
        assert _maxabs(x) < 1 << 29, "fq29_mul2 needs |limb| < 2^29 on all four operands"
    return mul_closed(F, [(a, b), (c, d)])


# ---------------------------------------------------------------- group formulas: g1_29.h itself, run on the model
# The straight-line formulas are not restated here: their C text is read from csrc/g1_29.h and executed statement by
# statement on limb lists, with fq29_mul / fq29_sqr / fq29_mul2 replaced by the model products that assert their budget
# first.  A formula that loses a fq29_norm, or gains a product outside the budget, fails here even where the C result
# still comes out right.
class _NS:
    def __init__(self, rec=None):
        if rec is not None:
            self.x, self.y, self.zz, self.zzz = rec

    def rec(self):
        return [self.x, self.y, self.zz, self.zzz]


def _split_top(s):
    parts, depth, cur = [], 0, ""
    for ch in s:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return parts + [cur]


# name -> (parameters taken, values returned)
_FORMULAS = {"xyzz29_finish": (5, ["pp", "ppp"]), "xyzz29_madd_fast": (2, ["acc"]), "xyzz29_add_fast": (2, ["acc"]),
             "xyzz29_double": (1, None), "jac29_double": (3, ["x", "y", "z"]), "jac29_to_xyzz": (3, None)}


def _translate(src, name):
    import re

    m = re.search(r"^SNARKV_HD [\w ]+ %s\((.*?)\) \{\n(.*?)^\}" % name, src, re.S | re.M)
    assert m, name
    ntake, outs = _FORMULAS[name]
    params = [re.findall(r"\w+", p)[-1] for p in _split_top(m.group(1))][:ntake]
    lines = ["def %s(%s):" % (name, ", ".join(params))]
    for raw in m.group(2).split("\n"):
        st = raw.split("//")[0].strip()
        if not st:
            continue
        assert st.endswith(";") and not st.startswith(("if", "for", "while", "#")), "not straight-line code: " + st
        st = st[:-1]
        d = re.match(r"^(Fq29|G1Xyzz29) (.*)$", st)
        f = re.match(r"^xyzz29_finish\((.*), (\w+), (\w+)\)$", st)
        if d:
            for part in _split_top(d.group(2)):
                if "=" in part:
                    lines.append("    " + part.strip())
                elif d.group(1) == "G1Xyzz29":
                    lines.append("    %s = _NS()" % part.strip())
        elif f:
            lines.append("    %s, %s = xyzz29_finish(%s)" % (f.group(2), f.group(3), f.group(1)))
        else:
            lines.append("    " + st)
    if outs:
        lines.append("    return " + ", ".join(outs))
    return "\n".join(lines)


def formulas(F):
    """{name: python function} for the formulas of g1_29.h over the field F"""
    key = (F.q, "formulas")
    if key in _CACHE:
        return _CACHE[key]
    src = open(os.path.join(ROOT, "snark-verifier_amd", "csrc", "g1_29.h")).read()
    env = {"_NS": _NS, "fq29_mul": lambda a, b: m_mul(F, a, b), "fq29_sqr": lambda a: m_sqr(F, a),
           "fq29_mul2": lambda a, b, c, d: m_mul2(F, a, b, c, d), "fq29_norm": l_norm, "fq29_sub": l_sub, "fq29_add": l_add,
           "fq29_dbl": l_dbl, "fq29_neg": l_neg}
    for name in _FORMULAS:
        exec(_translate(src, name), env)
    _CACHE[key] = env
    return env


def m_madd_fast(F, acc, p):
    a, b = _NS(acc), _NS()
    b.x, b.y = p
    return formulas(F)["xyzz29_madd_fast"](a, b).rec()


def m_add_fast(F, acc, b):
    return formulas(F)["xyzz29_add_fast"](_NS(acc), _NS(b)).rec()


def m_double(F, pt):
    return formulas(F)["xyzz29_double"](_NS(pt)).rec()


def m_jac_double(F, x, y, z):
    return formulas(F)["jac29_double"](x, y, z)


def m_jac_to_xyzz(F, x, y, z):
    return formulas(F)["jac29_to_xyzz"](x, y, z).rec()


def m_to_affine(F, pt):
    """xyzz29_to_affine of a non-degenerate record: each coordinate is the OUTPUT of a product (not canonicalised)"""
    x, y, zz, zzz = pt
    zn = l_norm(m_mul(F, zz, zzz))
    inv = pow(val(zn) * F.rinv % F.q, -1, F.q)
    i = m_mul(F, spell(inv), spell(F.R * F.R % F.q))
    return [m_mul(F, x, m_mul(F, i, zzz)), m_mul(F, l_norm(y), m_mul(F, i, zz))]


def m_double_n(F, pt, n):
    if n <= 0:
        return pt
    x = m_mul(F, pt[0], pt[2])
    y = m_mul(F, l_norm(pt[1]), pt[3])
    z = pt[2]
    for _ in range(n):
        x, y, z = m_jac_double(F, x, y, z)
    return m_jac_to_xyzz(F, x, y, z)


# ---------------------------------------------------------------- what a record represents
def point_of_xyzz(C, rec):
    """affine point (plain integers) a raw XYZZ record stands for; None for ZZ = 0 (mod p).  Also checks ZZ^3 = ZZZ^2."""
    q, F = C.fq.q, C.fq
    x, y, zz, zzz = (val(c) for c in rec)
    if zz % q == 0:
        return None
    assert (zz ** 3 - zzz ** 2 * F.R) % q == 0, "ZZ^3 != ZZZ^2"
    return (x * pow(zz, -1, q) % q, y * pow(zzz, -1, q) % q)


def point_of_jac(C, x, y, z):
    q, F = C.fq.q, C.fq
    x, y, z = val(x) * F.rinv % q, val(y) * F.rinv % q, val(z) * F.rinv % q
    if z == 0:
        return None
    zi = pow(z, -1, q)
    return (x * zi * zi % q, y * zi * zi * zi % q)


def affine_rec(C, pt):
    """Montgomery affine record (canonical limbs), identity = all zero"""
    if pt is None:
        return [[0] * 9, [0] * 9]
    F = C.fq
    return [spell(pt[0] * F.R % F.q), spell(pt[1] * F.R % F.q)]


def in_closed_set(C, rec):
    """The accumulator set of the header of g1_29.h.  Returns None if inside, else what is wrong."""
    q = C.fq.q
    x, y, zz, zzz = rec
    if not (is_norm(x) and -4 * q < val(x) < 2 * q):
        return "x: carry-normalised in (-4p, 2p) violated: %.3f p" % (val(x) / q)
    if not (_maxabs(y[:8]) < 1 << 29 and -2 * q < val(y) < 2 * q):
        return "y: |limb| < 2^29 in (-2p, 2p) violated: %.3f p" % (val(y) / q)
    for n, c in (("zz", zz), ("zzz", zzz)):
        if not (is_norm(c) and -q // 4 < val(c) < 5 * q // 4):
            return "%s: product output in (-p/4, 5p/4) violated: %.3f p" % (n, val(c) / q)
    return None


# ---------------------------------------------------------------- operand generators (seeded)
def _low_limbs(rnd, cap, signed, extra=()):
    """limbs 0..7: per limb from {0, 1, 2^29 - 1, 2^29, cap, extras, random} (and negations when `signed`), capped"""
    pal = [v for v in (0, 1, MASK, 1 << 29, cap) + tuple(extra) if v <= cap]
    mode = rnd.randrange(4)

    def sg(v):
        return -v if signed and rnd.random() < 0.5 else v

    if mode == 0:
        return [sg(rnd.randrange(cap + 1)) for _ in range(8)]
    if mode == 1:
        return [sg(rnd.choice(pal)) for _ in range(8)]
    if mode == 2:  # all limbs equal in magnitude: all +, all -, alternating
        v = rnd.choice(pal)
        pat = rnd.randrange(4) if signed else 0
        return [v if pat == 0 else -v if pat == 1 else v * (-1) ** (i + pat) for i in range(8)]
    return [sg(rnd.choice(pal)) if rnd.random() < 0.5 else sg(rnd.randrange(cap + 1)) for _ in range(8)]


def targets(F, rnd):
    """(value to land next to, from which side): the edges of the lazy contract and of the accumulator set"""
    q = F.q
    t = [(8 * q, -1), (-8 * q, 1), (2 * q, -1), (-4 * q, 1), (-2 * q, 1), (0, 1), (0, -1), (1, 1), (-1, -1), (q, -1), (q, 1),
         (-q, 1), (-q, -1), (q + 1, 1), (q - 1, -1), (F.one, 1), (F.one, -1)]
    return t + [(rnd.randrange(-8 * q + 1, 8 * q), rnd.choice((1, -1))) for _ in range(8)]


def land(low, target, side, F):
    """limb 8 such that the value is the nearest one to `target` on the given side (+1: >= target, -1: <= target), then
    pulled strictly inside (-8p, 8p)"""
    lo = val(low)
    l8 = -((lo - target) >> 232) if side > 0 else (target - lo) >> 232
    v = lo + (l8 << 232)
    while v >= 8 * F.q:
        l8, v = l8 - 1, v - (1 << 232)
    while v <= -8 * F.q:
        l8, v = l8 + 1, v + (1 << 232)
    return low + [l8]


def respell(rnd, l, density=0.5):
    """another spelling of the same value with |limb| <= 2^29 - 1: borrow 2^29 from the next limb where the limb is >= 1"""
    l = list(l)
    for i in range(8):
        if l[i] > MASK:  # a carry pushed it to 2^29: must borrow
            l[i] -= 1 << 29
            l[i + 1] += 1
        elif l[i] >= 1 and rnd.random() < density:
            l[i] -= 1 << 29
            l[i + 1] += 1
    return l


def operand_pool(F, seed, n, kind):
    """n limb records of one class.  kind: 'norm' (carry-normalised), 'lazy' (|limb| <= 2^29), 'mid' (<= 2^29.8),
    'wide' (<= 2^30.6).  The value of each lies strictly inside (-8p, 8p), next to one of `targets`."""
    rnd = random.Random(seed)
    cap, signed, extra = {"norm": (MASK, False, ()), "lazy": (1 << 29, True, ()), "mid": (W298, True, ()),
                          "wide": (W306, True, ((1 << 30) - 1,))}[kind]
    out = []
    # the all-limbs-equal corners first, each on every target
    corners = [[cap] * 8] + ([[-cap] * 8, [cap * (-1) ** i for i in range(8)], [-cap * (-1) ** i for i in range(8)]] if signed else [[0] * 8])
    tg = targets(F, rnd)
    for c in corners:
        for t, s in tg:
            out.append(land(list(c), t, s, F))
    # exact edge values in three spellings: normalised, all limbs <= 0, mixed
    for v in (0, 1, -1, F.q, -F.q, F.q + 1, F.q - 1, F.one, 8 * F.q - 1, -8 * F.q + 1):
        out.append(spell(v))
        if signed:
            out.append(l_neg(spell(-v)))
            out.append(respell(rnd, spell(v)))
    while len(out) < n:
        t, s = rnd.choice(tg)
        out.append(land(_low_limbs(rnd, cap, signed, extra), t, s, F))
    out = out[:n]
    for l in out:  # the precondition, asserted on every record
        assert -8 * F.q < val(l) < 8 * F.q and _maxabs(l) <= cap
        if kind == "norm":
            assert is_norm(l)
    return np.array(out, dtype=np.int64).astype(np.int32)


def budget_mask(F, a, b):
    """vectorised `budget_ok` for (n, 9) arrays"""
    a, b = np.abs(a.astype(np.int64)), np.abs(b.astype(np.int64))
    ok = np.ones(len(a), dtype=bool)
    p = F.limbs
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        se = np.zeros(len(a), dtype=object)
        for i in range(lo, hi + 1):
            se = se + a[:, i].astype(object) * b[:, k - i].astype(object)
        red = MASK * sum(p[k - i] for i in range(lo, hi + 1)) + (1 << 35)
        ok &= np.array([x + red < (1 << 63) for x in se], dtype=bool)
    return ok


# ---------------------------------------------------------------- checks of product-like outputs
def check_product(F, out, t, what):
    """properties 1-3 of a product output: `out` (n, 9) int32, `t` object array of the exact integers sum a*b.
    residue: val(out) 2^261 = t (mod q); shape: limbs 0..7 in [0, 2^29), limb 8 far inside int32;
    range: 0 <= val(out) 2^261 - t < q 2^261."""
    out = np.asarray(out)
    assert out.shape == (len(t), 9), what
    assert ((out[:, :8] >= 0) & (out[:, :8] <= MASK)).all(), what + ": a limb 0..7 outside [0, 2^29)"
    assert (np.abs(out[:, 8].astype(np.int64)) < (1 << 26)).all(), what + ": limb 8 too large"
    d = vals(out) * F.R - t
    bad = [i for i, x in enumerate(d) if x % F.q != 0]
    assert not bad, "%s: residue wrong at %d elements, first %d" % (what, len(bad), bad[0])
    bad = [i for i, x in enumerate(d) if not 0 <= x < F.q * F.R]
    assert not bad, "%s: value outside a*b/2^261 + [0, q) at %d elements, first %d" % (what, len(bad), bad[0])
    return len(t)


# ---------------------------------------------------------------- section 3a: the field layer, element-wise
_CACHE = {}


def _pool(F, seed, n, kind):
    key = (F.q, seed, n, kind)
    if key not in _CACHE:
        _CACHE[key] = operand_pool(F, seed, n, kind)
    return _CACHE[key]


def _residues(F, rnd, n, extra=()):
    q = F.q
    edge = [0, 1, 2, q - 1, q - 2, F.one, (1 << 256) % q, (1 << 232) - 1, 1 << 232, (q - 1) // 2] + list(extra)
    return (edge + [rnd.randrange(q) for _ in range(n)])[:n]


def kp_spellings(F, seed):
    """every k q and k q +- 1 for |k| <= 8 (the outermost pair sits ON the edge of the lazy contract) in several limb
    spellings of the same value: normalised, all limbs <= 0, borrows parked in the middle limbs, a wide limb"""
    rnd = random.Random(seed)
    out = []
    for k in range(-8, 9):
        for d in (0, 1, -1):
            v = k * F.q + d
            sp = [spell(v), l_neg(spell(-v)), respell(rnd, spell(v)), respell(rnd, spell(v), 1.0)]
            w = spell(v)
            w[3] += 3 << 29  # a carry parked in a middle limb
            w[4] -= 3
            sp.append(w)
            w = l_neg(spell(-v))
            w[5] -= 2 << 29
            w[6] += 2
            sp.append(w)
            for l in sp:
                assert val(l) == v
                out.append(l)
    return np.array(out, dtype=np.int64).astype(np.int32)


def field_cases(C, n=50000):
    """op -> (n_op, words in) int32 input array; every record inside the contract of its operation (asserted here)"""
    key = (C.name, "field", n)
    if key in _CACHE:
        return _CACHE[key]
    F, Fr = C.fq, C.fr
    rnd = random.Random(2929)
    cases = {}
    norm, norm2 = _pool(F, 1, n, "norm"), _pool(F, 2, n, "norm")
    lazy, mid, mid2, wide = _pool(F, 3, n, "lazy"), _pool(F, 4, n, "mid"), _pool(F, 5, n, "mid"), _pool(F, 6, n, "wide")
    t = n // 4
    # (normalised, wide), (wide, normalised), (both <= 2^29.8), (|limb| <= 2^29 lazy, wide)
    a = np.concatenate([norm[:t], wide[t:2 * t], mid[2 * t:3 * t], lazy[3 * t:]])
    b = np.concatenate([wide[:t], norm[t:2 * t], mid2[2 * t:3 * t], wide[3 * t:]])
    cases["fq29_mul"] = np.concatenate([a, b], axis=1)
    cases["fq29_sqr"] = norm
    nneg, nneg2 = -norm2, -_pool(F, 7, n, "norm")
    h = n // 2
    cases["fq29_mul2"] = np.concatenate([np.concatenate([norm[:h], nneg2[h:]]), np.concatenate([nneg[:h], norm2[h:]]),
                                         np.concatenate([nneg2[:h], norm[h:]]), np.concatenate([norm2[:h], nneg[h:]])], axis=1)
    cases["fq29_norm"] = np.concatenate([wide[:h], lazy[h:]])
    q = F.q
    cop = [-q + 1, -1, 0, 1, q - 1, q, q + 1, 2 * q - 1, -q // 8, q + q // 8] + [rnd.randrange(-q + 1, 2 * q) for _ in range(n)]
    cases["fq29_canon_of_product"] = np.array([spell(v) for v in cop[:n]], dtype=np.int64).astype(np.int32)
    kp = kp_spellings(F, 8)
    cases["fq29_canon_residue"] = np.concatenate([kp, wide, lazy])[:max(n, len(kp))]
    cases["fq29_is_zero_mod_p"] = cases["fq29_canon_residue"]
    res = _residues(F, rnd, n)
    cases["fq29_from_words"] = np.array([words_i32(v) for v in res], dtype=np.int32)
    cases["fq29_from_words_mont"] = cases["fq29_from_words"]
    cases["fq29_to_words"] = np.concatenate([lazy[:h], wide[h:]])
    cases["fq29_to_words_mont"] = cases["fq29_to_words"]
    cases["fq29_pack256"] = np.array([spell(v) for v in res], dtype=np.int32)
    cases["fq29_unpack256"] = cases["fq29_from_words"]
    rn, rw, rm, rm2 = _pool(Fr, 11, n, "norm"), _pool(Fr, 12, n, "wide"), _pool(Fr, 13, n, "mid"), _pool(Fr, 14, n, "mid")
    cases["fr29_mul"] = np.concatenate([np.concatenate([rn[:h], rm[h:]]), np.concatenate([rw[:h], rm2[h:]])], axis=1)
    # a b + c d at the corner of its budget, 27 products per column: every operand carry-normalised or the limb-wise negation
    # of that, in all sixteen sign patterns; the pools open with limbs 0..7 all at 2^29 - 1, so the first sixteen records are
    # that corner in every pattern
    sign = np.array([[1 - 2 * ((i >> j) & 1) for j in range(4)] for i in range(16)], dtype=np.int32)[np.arange(n) % 16]
    cases["fr29_mul2"] = np.concatenate([_pool(Fr, s, n, "norm") * sign[:, j:j + 1] for j, s in enumerate((11, 16, 17, 19))],
                                        axis=1)
    assert (np.abs(cases["fr29_mul2"][:16].reshape(-1, 9)[:, :8]) == MASK).all(), "the corner of the fr29_mul2 budget is missing"
    # the codecs: 0, 1, r - 1 and uniform residues in; out, every k r and k r +- 1 up to the +-8r of the lazy contract
    cases["fr29_from_canonical"] = np.array([words_i32(v) for v in _residues(Fr, random.Random(2930), n)], dtype=np.int32)
    cases["fr29_to_canonical"] = np.concatenate([kp_spellings(Fr, 18), rm[:h], rw[h:]])[:n]
    cases["fr29_pow5"] = rm
    cases["fr29_canon_residue"] = np.concatenate([kp_spellings(Fr, 15), rw])[:n]
    # 8 x 32: all-ones clipped below p, p - 1, single bits, random
    e32 = [min((1 << 256) - 1, q - 1), q - 1, q - 2, 0, 1] + [1 << i for i in range(q.bit_length() - 1)]
    e32 += [min(int.from_bytes(bytes([0xFF] * 4 * j + [0] * (32 - 4 * j)), "little"), q - 1) for j in range(1, 9)]
    xa = [rnd.choice(e32) if i % 3 == 0 else rnd.randrange(q) for i in range(n)]
    xb = [rnd.choice(e32) if i % 5 < 2 else rnd.randrange(q) for i in range(n)]
    xa[:len(e32)] = e32
    xb[:len(e32)] = e32[::-1]
    cases["fq_mul"] = np.array([words_i32(x) + words_i32(y) for x, y in zip(xa, xb)], dtype=np.int32)
    # the preconditions that the pools do not already assert
    A, B = cases["fq29_mul"][:, :9], cases["fq29_mul"][:, 9:]
    mx = np.abs(A.astype(np.int64)).max(axis=1).astype(object) * np.abs(B.astype(np.int64)).max(axis=1).astype(object)
    assert all(x <= 2 ** 59.6 for x in mx), "a product pair outside the operand classes"
    assert budget_mask(F, A, B).all(), "a product pair outside the column budget"
    A, B = cases["fr29_mul"][:, :9], cases["fr29_mul"][:, 9:]
    assert budget_mask(Fr, A, B).all()
    assert (np.abs(cases["fq29_mul2"].astype(np.int64)) < (1 << 29)).all()
    assert (np.abs(cases["fr29_mul2"].astype(np.int64)) < (1 << 29)).all()
    for name, arr in cases.items():
        assert arr.shape[1] == OPS[name][0] and len(arr) >= n, name
    _CACHE[key] = cases
    return cases


def _canon_expect(F, arr):
    return np.array([spell(v % F.q) for v in vals(arr)], dtype=np.int64).astype(np.int32)


def _eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d records differ, first at %d: %s != %s" % (
        what, len(bad), len(got), bad[0], got[bad[0]].tolist(), exp[bad[0]].tolist())
    return len(got)


def field_suite(C, run, n=50000, model_rows=2000):
    """Runs every field operation over `field_cases` through `run(op, in) -> out` and checks each record against exact
    integers.  Returns ({op: output array}, {op: records checked}); the caller asserts generated == checked."""
    F, Fr = C.fq, C.fr
    cases = field_cases(C, n)
    outs, checked = {}, {}
    for name, inp in cases.items():
        outs[name] = np.asarray(run(name, inp))
        assert outs[name].shape == (len(inp), OPS[name][1]), name
    # products: residue, shape, range, and the model's nine limbs
    for name, fld, npairs in (("fq29_mul", F, 1), ("fq29_sqr", F, 0), ("fq29_mul2", F, 2), ("fr29_mul", Fr, 1),
                              ("fr29_mul2", Fr, 2)):
        inp = cases[name]
        if npairs == 0:
            v = vals(inp)
            t = v * v
        else:
            t = sum(vals(inp[:, 18 * j:18 * j + 9]) * vals(inp[:, 18 * j + 9:18 * j + 18]) for j in range(npairs))
        checked[name] = check_product(fld, outs[name], t, "%s %s" % (C.name, name))
        exp = np.array([spell((x + ((x * fld.nqinv) % fld.R) * fld.q) >> RBITS) for x in t], dtype=np.int64).astype(np.int32)
        _eq(outs[name], exp, "%s %s against the closed form" % (C.name, name))
        rows = inp[:model_rows].tolist()
        for i, r in enumerate(rows):  # the column loop itself, with its accumulator watched
            pairs = [(r, r)] if npairs == 0 else [(r[18 * j:18 * j + 9], r[18 * j + 9:18 * j + 18]) for j in range(npairs)]
            lim, _ = mul_columns(fld, pairs)
            assert lim == outs[name][i].tolist(), "%s %s: column model differs at %d" % (C.name, name, i)
    # norm: same value, carry-normalised
    o = outs["fq29_norm"]
    assert ((o[:, :8] >= 0) & (o[:, :8] <= MASK)).all()
    assert (vals(o) == vals(cases["fq29_norm"])).all()
    checked["fq29_norm"] = len(o)
    checked["fq29_canon_of_product"] = _eq(outs["fq29_canon_of_product"], _canon_expect(F, cases["fq29_canon_of_product"]),
                                           C.name + " fq29_canon_of_product")
    checked["fq29_canon_residue"] = _eq(outs["fq29_canon_residue"], _canon_expect(F, cases["fq29_canon_residue"]),
                                        C.name + " fq29_canon_residue")
    z = np.array([[1 if v % F.q == 0 else 0] for v in vals(cases["fq29_is_zero_mod_p"])], dtype=np.int32)
    assert z.sum() >= 17 * 6, "the k p spellings are missing"
    checked["fq29_is_zero_mod_p"] = _eq(outs["fq29_is_zero_mod_p"], z, C.name + " fq29_is_zero_mod_p")
    checked["fr29_canon_residue"] = _eq(outs["fr29_canon_residue"], _canon_expect(Fr, cases["fr29_canon_residue"]),
                                        C.name + " fr29_canon_residue")
    # codecs
    w = [int_of_words(r) for r in cases["fq29_from_words"].tolist()]
    for name, const in (("fq29_from_words", F.R * F.R % F.q), ("fq29_from_words_mont", (1 << 266) % F.q)):
        t = np.array([x * const for x in w], dtype=object)
        checked[name] = check_product(F, outs[name], t, "%s %s" % (C.name, name))
    for name, const in (("fq29_to_words", F.rinv), ("fq29_to_words_mont", F.rinv * (1 << 256) % F.q)):
        exp = np.array([words_i32(v * const % F.q) for v in vals(cases[name])], dtype=np.int32)
        checked[name] = _eq(outs[name], exp, "%s %s" % (C.name, name))
    exp = np.array([words_i32(v) for v in vals(cases["fq29_pack256"])], dtype=np.int32)
    checked["fq29_pack256"] = _eq(outs["fq29_pack256"], exp, C.name + " fq29_pack256")
    exp = np.array([spell(x) for x in w], dtype=np.int32)
    checked["fq29_unpack256"] = _eq(outs["fq29_unpack256"], exp, C.name + " fq29_unpack256")
    w = np.array([int_of_words(r) * (Fr.R * Fr.R % Fr.q) for r in cases["fr29_from_canonical"].tolist()], dtype=object)
    checked["fr29_from_canonical"] = check_product(Fr, outs["fr29_from_canonical"], w, C.name + " fr29_from_canonical")
    exp = np.array([words_i32(v * Fr.rinv % Fr.q) for v in vals(cases["fr29_to_canonical"])], dtype=np.int32)
    checked["fr29_to_canonical"] = _eq(outs["fr29_to_canonical"], exp, C.name + " fr29_to_canonical")
    # x^5 through three products, limb for limb
    exp = []
    for r in cases["fr29_pow5"].tolist():
        x2 = m_mul(Fr, r, r)
        exp.append(m_mul(Fr, m_mul(Fr, x2, x2), r))
    checked["fr29_pow5"] = _eq(outs["fr29_pow5"], np.array(exp, dtype=np.int32), C.name + " fr29_pow5")
    d = vals(outs["fr29_pow5"]) * (Fr.R ** 4) - vals(cases["fr29_pow5"]) ** 5
    assert all(x % Fr.q == 0 for x in d)
    # 8 x 32 Montgomery product, R = 2^256
    ri = pow(1 << 256, -1, F.q)
    exp = np.array([words_i32(int_of_words(r[:8]) * int_of_words(r[8:]) * ri % F.q) for r in cases["fq_mul"].tolist()],
                   dtype=np.int32)
    checked["fq_mul"] = _eq(outs["fq_mul"], exp, C.name + " fq_mul")
    for name in cases:  # no class dropped: generated == checked, and at least n of each
        assert checked[name] == len(cases[name]) >= n, name
    return outs, checked


# ---------------------------------------------------------------- section 3b: accumulators at the corners of their set
# Two sets of raw XYZZ records, both stated in the header of g1_29.h:
#   S   what an adder or xyzz29_double leaves: x carry-normalised in (-4p, 2p); y with |limb| < 2^29 in (-2p, 2p);
#       zz, zzz product outputs (carry-normalised, (-p/4, 5p/4))                                   -> `in_closed_set`
#   SJ  what a Jacobian doubling chain leaves (jac29_to_xyzz): x carry-normalised in (-6p, 11p), y carry-normalised in
#       (-9.5p, 2p), zz, zzz as in S; the chain itself keeps x, y in those intervals and z in (-p/2, 5p/2) -> `in_jac_set`
# The intervals of SJ follow from the product range a*b/2^261 + [0, p) with 2^261/p >= 128 (pallas, the tighter curve):
# for x in (-6p, 11p), y in (-9.5p, 2p), z in (-p/2, 5p/2):  A = X^2 < 1.95p, B = Y^2 < 1.71p, C = B^2 < 1.03p;
# (X+B)^2 - A - C = 2XB/2^261 + (m1 - m2 - m3) p with |2XB|/2^261 < 0.29p, so D in (-4.6p, 2.6p); E = 3A < 5.85p;
# F = E^2 < 1.27p; X3 = F - 2D in (-5.2p, 10.5p); E(D - X3) in (-0.69p, 1.69p), 8C < 8.19p: Y3 in (-8.9p, 1.69p);
# Z3 = 2YZ in (-0.37p, 2.37p).  Each lies inside the interval it started from.
def in_jac_set(C, x, y, z):
    q = C.fq.q
    for n, c, lo, hi in (("x", x, -6, 11), ("y", y, -9.5, 2), ("z", z, -0.5, 2.5)):
        if not (is_norm(c) and lo * q < val(c) < hi * q):
            return "Jacobian %s: carry-normalised in (%sp, %sp) violated: %.3f p" % (n, lo, hi, val(c) / q)
    return None


def in_chain_output_set(C, rec):
    q = C.fq.q
    x, y, zz, zzz = rec
    if not (is_norm(x) and -6 * q < val(x) < 11 * q):
        return "x of a chain output outside (-6p, 11p): %.3f p" % (val(x) / q)
    if not (is_norm(y) and -9.5 * q < val(y) < 2 * q):
        return "y of a chain output outside (-9.5p, 2p): %.3f p" % (val(y) / q)
    for n, c in (("zz", zz), ("zzz", zzz)):
        if not (is_norm(c) and -q // 4 < val(c) < 5 * q // 4):
            return "%s: product output in (-p/4, 5p/4) violated: %.3f p" % (n, val(c) / q)
    return None


def base_points(C, n, seed=5):
    key = (C.name, "pts", n, seed)
    if key not in _CACHE:
        rnd = random.Random(seed)
        _CACHE[key] = [C.O.g1_mul(C.O.G1_GEN, rnd.randrange(1, C.O.R)) for _ in range(n)]
    return _CACHE[key]


def _spell_n(F, res, want):
    """a product-output spelling of the residue: 0: res, 1: res + p (needs res < p/4), 2: res - p (needs res > 3p/4)"""
    q = F.q
    if want == 1 and res + q < 5 * q // 4:
        return spell(res + q)
    if want == 2 and res - q > -q // 4:
        return spell(res - q)
    return None if want else spell(res)


def _y_spelling(rnd, v, mode):
    return [spell(v), l_neg(spell(-v)), respell(rnd, spell(v)), respell(rnd, spell(v), 1.0)][mode]


def make_acc(C, rnd, pt, kx, ky, ymode, zzw, zzzw, chain=False):
    """A raw XYZZ record for the affine point `pt` (plain integers): x spelled as residue + kx p, y as residue + ky p in
    one of four limb spellings, zz / zzz in the wanted product-output spelling (z is redrawn until that spelling exists)"""
    F = C.fq
    q = F.q
    for _ in range(4000):
        z = rnd.randrange(1, q)
        zz, zzz = z * z % q, z * z * z % q
        lzz, lzzz = _spell_n(F, zz * F.R % q, zzw), _spell_n(F, zzz * F.R % q, zzzw)
        if lzz is not None and lzzz is not None:
            break
    else:
        raise AssertionError("no z found")
    X, Y = pt[0] * zz * F.R % q, pt[1] * zzz * F.R % q
    lx = spell(X + kx * q)
    ly = spell(Y + ky * q) if chain else _y_spelling(rnd, Y + ky * q, ymode)
    return [lx, ly, lzz, lzzz]


def corner_accs(C, n, seed, chain=False):
    """n (record, point) pairs that cover every x / y multiple of p of the set, every spelling of y, every spelling of
    zz and zzz; each record is asserted to lie inside its set and to represent its point"""
    key = (C.name, "accs", n, seed, chain)
    if key in _CACHE:
        return _CACHE[key]
    rnd = random.Random(seed)
    pts = base_points(C, 48)
    q = C.fq.q
    out = []
    i = 0
    while len(out) < n:
        pt = pts[i % len(pts)]
        if chain:
            kx, ky = -6 + i % 17, -10 + (i // 17) % 12
        else:
            kx, ky = -4 + i % 6, -2 + (i // 6) % 4
        rec = make_acc(C, rnd, pt, kx, ky, (i // 24) % 4, (i // 3) % 3, (i // 9) % 3, chain)
        i += 1
        bad = in_chain_output_set(C, rec) if chain else in_closed_set(C, rec)
        if bad:  # residue + k p fell off the end of the interval (x residue 0 with k = -4, ...)
            assert i < 40 * n
            continue
        assert point_of_xyzz(C, rec) == pt
        out.append((rec, pt))
    _CACHE[key] = out
    return out


def flat(*recs):
    return [x for r in recs for l in r for x in l]


def unflat(row, k):
    return [list(row[9 * i:9 * i + 9]) for i in range(k)]


def _arr(rows):
    return np.array(rows, dtype=np.int64).astype(np.int32)


def _other(rnd, pool, pt, C):
    while True:
        rec, q = rnd.choice(pool)
        if q[0] != pt[0]:
            return rec, q


def jac_corners(C, n, seed=23):
    """n ((x, y, z), point): Jacobian records at the corners of the chain's set `in_jac_set`"""
    key = (C.name, "jac", n, seed)
    if key in _CACHE:
        return _CACHE[key]
    F = C.fq
    q = F.q
    rnd = random.Random(seed)
    pts = base_points(C, 48)
    out, i = [], 0
    while len(out) < n:
        pt = pts[i % len(pts)]
        z = rnd.randrange(1, q)
        lz = spell(z * F.R % q + ((i // 7) % 3) * q)
        lx = spell(pt[0] * z * z * F.R % q + (-6 + i % 17) * q)
        ly = spell(pt[1] * z * z * z * F.R % q + (-10 + (i // 17) % 12) * q)
        i += 1
        assert i < 40 * n
        if in_jac_set(C, lx, ly, lz) is None:  # else this corner does not exist for this residue
            assert point_of_jac(C, lx, ly, lz) == pt
            out.append(([lx, ly, lz], pt))
    _CACHE[key] = out
    return out


def jac_corner_rows(C, n):
    return _arr([flat(j) + [1] for j, _ in jac_corners(C, n)])


def closure_suite(C, run, n_acc=2000, per=3):
    """Every adder / doubling applied ONCE to every corner accumulator: (i) the point it represents is the oracle's,
    (ii) the raw output is inside the set again, (iii) the step recomputed in the model (which asserts the limb budget
    before each product) gives the same limbs.  Returns {op: (generated, checked)}."""
    F, O = C.fq, C.O
    rnd = random.Random(31)
    S = corner_accs(C, n_acc, 21)
    SJ = corner_accs(C, max(n_acc // 4, 200), 22, chain=True)
    aff = [(affine_rec(C, p), p) for p in base_points(C, 48)]
    count = {}

    def go(op, rows, meta, model, oracle, inset, nrec=4):
        out = np.asarray(run(op, _arr(rows))).tolist()
        done = 0
        for row_in, row_out, (a, pa, b, pb) in zip(rows, out, meta):
            got = unflat(row_out, nrec)
            what = "%s %s #%d" % (C.name, op, done)
            assert got == model(a, b), what + ": limbs differ from the model"
            bad = inset(got)
            assert bad is None, what + ": " + bad
            assert point_of_xyzz(C, got) == oracle(pa, pb), what + ": wrong point"
            done += 1
        count[op] = (len(rows), done)

    rows, meta = [], []
    for rec, pt in S:
        for _ in range(per):
            b, pb = _other(rnd, aff, pt, C)
            rows.append(flat(rec, b))
            meta.append((rec, pt, b, pb))
    go("xyzz29_madd_fast", rows, meta, lambda a, b: m_madd_fast(F, a, b), O.g1_add, lambda r: in_closed_set(C, r))
    # the careful adder on the same non-exceptional inputs must give the same limbs
    out_c = np.asarray(run("xyzz29_madd_careful", _arr(rows)))
    out_f = np.asarray(run("xyzz29_madd_fast", _arr(rows)))
    count["xyzz29_madd_careful"] = (len(rows), _eq(out_c, out_f, C.name + " madd careful against fast"))
    rows, meta = [], []
    both = S + SJ
    for rec, pt in both:
        for _ in range(per):
            b, pb = _other(rnd, both, pt, C)
            rows.append(flat(rec, b))
            meta.append((rec, pt, b, pb))
    go("xyzz29_add_fast", rows, meta, lambda a, b: m_add_fast(F, a, b), O.g1_add, lambda r: in_closed_set(C, r))
    out_c = np.asarray(run("xyzz29_add_careful", _arr(rows)))
    out_f = np.asarray(run("xyzz29_add_fast", _arr(rows)))
    count["xyzz29_add_careful"] = (len(rows), _eq(out_c, out_f, C.name + " add careful against fast"))
    sk = np.asarray(run("xyzz29_add_skipid_fast", _arr([r + [0] for r in rows])))
    assert (sk[:, 36] == 0).all(), "skipid raised `bad` on an ordinary addition"
    count["xyzz29_add_skipid_fast"] = (len(rows), _eq(sk[:, :36], out_f, C.name + " add skipid against fast"))
    rows = [flat(rec) for rec, _ in S]
    meta = [(rec, pt, None, None) for rec, pt in S]
    go("xyzz29_double", rows, meta, lambda a, b: m_double(F, a), lambda p, _: O.g1_double(p), lambda r: in_closed_set(C, r))
    rows = [flat(rec) + [1] for rec, _ in S]
    go("xyzz29_double_n", rows, meta, lambda a, b: m_double_n(F, a, 1), lambda p, _: O.g1_double(p),
       lambda r: in_chain_output_set(C, r))
    # one Jacobian doubling on the corners of the chain's own set
    q = F.q
    meta = jac_corners(C, n_acc)
    rows = [flat(j) + [1] for j, _ in meta]
    out = np.asarray(run("jac29_double", _arr(rows))).tolist()
    xy = np.asarray(run("jac29_to_xyzz", _arr([r[:27] for r in rows]))).tolist()
    done = 0
    for row_out, row_xy, (j, pt) in zip(out, xy, meta):
        got = unflat(row_out, 3)
        what = "%s jac29_double #%d" % (C.name, done)
        assert got == list(m_jac_double(F, *j)), what + ": limbs differ from the model"
        bad = in_jac_set(C, *got)
        assert bad is None, what + ": " + bad
        assert point_of_jac(C, *got) == O.g1_double(pt), what + ": wrong point"
        r4 = unflat(row_xy, 4)
        assert r4 == m_jac_to_xyzz(F, *j) and in_chain_output_set(C, r4) is None and point_of_xyzz(C, r4) == pt, \
            "%s jac29_to_xyzz #%d" % (C.name, done)
        done += 1
    count["jac29_double"] = (len(rows), done)
    count["jac29_to_xyzz"] = (len(rows), done)
    # leaving the representation: xyzz29_to_affine / xyzz29_is_degenerate on every corner
    rows = [flat(rec) for rec, _ in both]
    ta = np.asarray(run("xyzz29_to_affine", _arr(rows)))
    exp = _arr([flat(m_to_affine(F, rec)) for rec, _ in both])
    count["xyzz29_to_affine"] = (len(rows), _eq(ta, exp, C.name + " xyzz29_to_affine"))
    for row, (_, pt) in zip(ta.tolist(), both):  # product outputs congruent to the Montgomery affine coordinates
        for c, want in zip(unflat(row, 2), affine_rec(C, pt)):
            assert is_norm(c) and -q // 4 < val(c) < 5 * q // 4 and val(c) % q == val(want)
    dg = np.asarray(run("xyzz29_is_degenerate", _arr(rows)))
    assert not dg.any()
    count["xyzz29_is_degenerate"] = (len(rows), len(dg))
    for op, (g, c) in count.items():
        assert g == c and g >= n_acc, op
    return count


# ---------------------------------------------------------------- exceptional inputs
def _neg_rec(rec):
    return [rec[0], l_neg(rec[1]), rec[2], rec[3]]


def _limbs_zero(l):
    return not any(l)


def exceptional_suite(C, run, n=2000):
    """P = +-Q and the identity through the three flavours of adder, the equal points in different spellings."""
    F, O = C.fq, C.O
    q = F.q
    rnd = random.Random(41)
    S = corner_accs(C, n, 21)
    pts = base_points(C, 48)
    same = {}
    for rec, pt in S:
        same.setdefault(pt, []).append(rec)
    aff = {pt: affine_rec(C, pt) for pt in pts}
    count = {}

    def degenerate(recs):
        return np.asarray(run("xyzz29_is_degenerate", _arr([flat(r) for r in recs])))[:, 0]

    def unrelated(pt):
        return _other(rnd, S, pt, C)[0]

    def twin_of(rec, pt, want):
        """another record of the same point whose u2 - u1 is want * p in the adder (on purpose: it is rare), else any"""
        for t in same[pt]:
            if (val(m_mul(F, t[0], rec[2])) - val(m_mul(F, rec[0], t[2]))) == want * q:
                return t
        return rnd.choice(same[pt])

    # ---- _fast: the ONE documented behaviour: ZZ = 0 (mod p) after the step and after three further additions
    rows_a, rows_m, classes = [], [], {}
    owners = []
    for i, (rec, pt) in enumerate(S):
        twin = twin_of(rec, pt, (0, 1, -1)[i % 3])
        for b in (twin, _neg_rec(twin), rec):
            rows_a.append(flat(rec, b))
            owners.append(pt)
            u1, u2 = m_mul(F, rec[0], b[2]), m_mul(F, b[0], rec[2])
            k, rem = divmod(val(u2) - val(u1), q)
            assert rem == 0
            classes[k] = classes.get(k, 0) + 1
    assert all(classes.get(k, 0) > 0 for k in (0, 1, -1)), "u2 - u1 in {0, p, -p} not all reached: %s" % classes
    assert set(classes) <= {0, 1, -1}
    for rec, pt in S:
        for a in (aff[pt], affine_rec(C, O.g1_neg(pt))):
            rows_m.append(flat(rec, a))
    cur = np.concatenate([np.asarray(run("xyzz29_add_fast", _arr(rows_a))), np.asarray(run("xyzz29_madd_fast", _arr(rows_m)))])
    first = cur.tolist()
    own = owners + [pt for _, pt in S for _ in range(2)]
    for row in first:  # the model's claim about the spelling of a degenerate ZZ: the integer 0 or the integer p
        assert val(row[18:27]) in (0, q), "degenerate ZZ is neither 0 nor p: %d" % val(row[18:27])
    for step in range(4):
        assert degenerate([unflat(r, 4) for r in cur.tolist()]).all(), "ZZ = 0 (mod p) lost after %d further additions" % step
        if step == 3:
            break
        if step % 2 == 0:
            cur = np.asarray(run("xyzz29_madd_fast", _arr([r + flat(aff[rnd.choice(pts)]) for r in cur.tolist()])))
        else:
            cur = np.asarray(run("xyzz29_add_fast", _arr([r + flat(unrelated(p)) for r, p in zip(cur.tolist(), own)])))
    count["fast_degenerate"] = (len(rows_a) + len(rows_m), len(cur))
    # leaving the representation: a degenerate record and the stored identity both come out as (0, 0)
    za = np.asarray(run("xyzz29_to_affine", _arr(first + [flat(i) for i in ([[0] * 9] * 4, [[3] * 9, [1] * 9, [0] * 9, [7] * 9])])))
    assert not za.any(), "xyzz29_to_affine of a degenerate record or the identity is not (0, 0)"
    count["to_affine_degenerate"] = (len(first) + 2, len(za))

    # ---- _careful: the whole table against the oracle
    ident = [[[0] * 9] * 4, [[5, 6, 7, 8, 9, 1, 2, 3, 4], [1] * 9, [0] * 9, [MASK] * 9]]  # zz all-zero limbs is the marker
    rows, exp, kind = [], [], []
    for rec, pt in S:
        twin = rnd.choice(same[pt])
        other, po = _other(rnd, S, pt, C)
        idn = ident[len(rows) % 2]
        for b, want, k in ((twin, O.g1_double(pt), "pt"), (rec, O.g1_double(pt), "pt"), (_neg_rec(twin), None, "id"),
                           (idn, rec, "same"), ):
            rows.append(flat(rec, b))
            exp.append(want)
            kind.append(k)
        rows.append(flat(idn, other))
        exp.append(other)
        kind.append("same")
        rows.append(flat(idn, ident[(len(rows) + 1) % 2]))
        exp.append(None)
        kind.append("id")

    def table(op, rows, exp, kind, skipid=False):
        out = np.asarray(run(op, _arr(rows))).tolist()
        for i, (row, want, k) in enumerate(zip(out, exp, kind)):
            got = unflat(row, 4)
            what = "%s %s case %d (%s)" % (C.name, op, i, k)
            if k == "pt":
                assert point_of_xyzz(C, got) == want and not _limbs_zero(got[2]), what
            elif k == "id":
                assert _limbs_zero(got[2]), what
            else:
                assert got == [list(c) for c in want], what
            if skipid:
                assert row[36] == 0, what + ": `bad` raised"
        return len(out)

    count["xyzz29_add_careful"] = (len(rows), table("xyzz29_add_careful", rows, exp, kind))
    keep = [i for i, k in enumerate(kind) if k != "pt" and not (k == "id" and rows[i][36 + 18:36 + 27] != [0] * 9)]
    count["xyzz29_add_skipid_fast"] = (len(keep), table("xyzz29_add_skipid_fast", [rows[i] + [0] for i in keep],
                                                        [exp[i] for i in keep], [kind[i] for i in keep], True))
    rows, exp, kind = [], [], []
    one = spell(F.one)
    for rec, pt in S:
        other = rnd.choice([p for p in pts if p[0] != pt[0]])
        idn = ident[len(rows) % 2]
        for acc, a, want, k in ((rec, aff[pt], O.g1_double(pt), "pt"), (rec, affine_rec(C, O.g1_neg(pt)), None, "id"),
                                (rec, [[0] * 9] * 2, rec, "same"), (idn, aff[other], aff[other] + [one, one], "same"),
                                (idn, [[0] * 9] * 2, idn, "same")):
            rows.append(flat(acc, a))
            exp.append(want)
            kind.append(k)
    count["xyzz29_madd_careful"] = (len(rows), table("xyzz29_madd_careful", rows, exp, kind))

    # ---- skipid_fast: what k_fixup / chunk_sums rely on.  After any sequence that contained an exceptional addition,
    # `bad` is set, or the final accumulator is degenerate and not the stored identity; never neither.
    rows, tails = [], []
    for i, (rec, pt) in enumerate(S):
        twin = twin_of(rec, pt, (1, -1, 0)[i % 3])
        for b in (twin, _neg_rec(twin), rec):
            rows.append(flat(rec, b) + [0])
            tails.append([rnd.choice([None, unrelated(pt)]) if j else unrelated(pt) for j in range(1 + len(rows) % 4)])
    cur = np.asarray(run("xyzz29_add_skipid_fast", _arr(rows))).tolist()
    spell_seen = {0: 0, q: 0}
    for row in cur:
        zz = val(row[18:27])
        assert zz in spell_seen, "skipid: degenerate ZZ is neither the integer 0 nor the integer p: %d" % zz
        spell_seen[zz] += 1
        assert (row[36] == 1) == (zz == 0 and _limbs_zero(row[18:27])), "skipid: `bad` must rise exactly on the integer 0"
    assert spell_seen[0] and spell_seen[q], "both spellings of a degenerate ZZ must occur: %s" % spell_seen
    for step in range(5):
        live = [i for i, t in enumerate(tails) if len(t) > step]
        if not live:
            break
        nxt = np.asarray(run("xyzz29_add_skipid_fast", _arr(
            [cur[i][:36] + flat(tails[i][step] or ident[0]) + [cur[i][36]] for i in live]))).tolist()
        for i, r in zip(live, nxt):
            cur[i] = r
    dg = degenerate([unflat(r, 4) for r in cur])
    for i, row in enumerate(cur):
        assert row[36] == 1 or (dg[i] and not _limbs_zero(row[18:27])), \
            "%s skipid sequence %d ends undetected (bad = 0, ZZ = %d)" % (C.name, i, val(row[18:27]))
    count["skipid_sequences"] = (len(rows), len(cur))
    for op, (g, c) in count.items():
        assert g == c and g >= n, op
    return count


# ---------------------------------------------------------------- section 3c: chains
CHAIN_N = (1, 2, 13, 16, 17, 127, 254)


def scalar_list(C, rnd):
    r = C.O.R
    return [0, 1, 2, r - 1, r, r + 1, 1 << 255, (1 << 256) - 1] + [rnd.randrange(r) for _ in range(4)]


def glv_rows(C):
    """the scalars of test_glv_split_is_exact_and_fits_127_bits (tests/test_curve_math_host.py)"""
    R = C.O.R
    rnd = random.Random(9)
    w = next(pow(g, (R - 1) // 3, R) for g in range(2, 40) if pow(g, (R - 1) // 3, R) != 1)
    lams = [w, w * w % R]  # lambda is one of the two primitive cube roots of unity: take both
    ks = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 127, (1 << 128) - 1, (1 << 253), (1 << 254) % R]
    ks += [x for lam in lams for x in (lam, R - lam, lam * 7 % R)]
    ks += [rnd.randrange(R) for _ in range(4000)]
    return _arr([words_i32(k) for k in ks]), ks


W3_DIGITS = 43  # kWinDigits of csrc/glv.h


def w3_rows():
    """127-bit magnitudes for the signed 3-bit recoder: the edges (0, 1, 4 = the largest digit kept, 5 = the smallest that
    carries, 2^127 - 1, every 3-bit field 0b100 resp. 0b101) and seeded random ones of every length"""
    rnd = random.Random(43)
    top = (1 << 127) - 1
    all4 = sum(4 << (3 * i) for i in range(43)) & top
    all5 = sum(5 << (3 * i) for i in range(43)) & top
    ms = [0, 1, 4, 5, top, all4, all5, 3, 7, 8, 1 << 126, (1 << 96) - 1, 1 << 96, 0xFFFFFFFF, 1 << 32]
    ms += [rnd.getrandbits(127) for _ in range(2000)]
    ms += [rnd.getrandbits(rnd.randrange(1, 128)) for _ in range(2000)]
    return _arr([words_i32(m)[:4] for m in ms]), ms


def w3_suite(run):
    """every digit within [-3, 4] and sum d_i 8^i the magnitude itself; returns (records in, records checked)"""
    rows, ms = w3_rows()
    out = np.asarray(run("glv_w3_digits", rows)).tolist()
    for m, d in zip(ms, out):
        assert len(d) == W3_DIGITS and all(-3 <= x <= 4 for x in d), "digit out of [-3, 4] for %#x: %r" % (m, d)
        assert sum(x << (3 * i) for i, x in enumerate(d)) == m, "digits of %#x do not sum to it: %r" % (m, d)
    return len(ms), len(out)


def chain_suite(C, run, npts=256, model_long=8):
    F, O = C.fq, C.O
    rnd = random.Random(51)
    S = corner_accs(C, max(npts, 256), 21)[:npts]
    count = {}
    for n in CHAIN_N:
        out = np.asarray(run("xyzz29_double_n", _arr([flat(rec) + [n] for rec, _ in S]))).tolist()
        k = pow(2, n, O.R)
        for i, (row, (rec, pt)) in enumerate(zip(out, S)):
            got = unflat(row, 4)
            what = "%s xyzz29_double_n n = %d point %d" % (C.name, n, i)
            bad = in_chain_output_set(C, got)
            assert bad is None, what + ": " + bad
            assert point_of_xyzz(C, got) == O.g1_mul(pt, k), what
            if n <= 17 or i < model_long:  # every step in the model: its budget assertions and its set
                assert got == m_double_n(F, rec, n), what + ": limbs differ from the model"
        count["xyzz29_double_n/%d" % n] = (len(S), len(out))
        one = spell(F.one)
        jin = [affine_rec(C, pt) + [one] for _, pt in S]
        out = np.asarray(run("jac29_double", _arr([flat(j) + [n] for j in jin]))).tolist()
        for i, (row, (_, pt)) in enumerate(zip(out, S)):
            got = unflat(row, 3)
            bad = in_jac_set(C, *got)
            assert bad is None, "%s jac29_double x %d point %d: %s" % (C.name, n, i, bad)
            assert point_of_jac(C, *got) == O.g1_mul(pt, k)
        count["jac29_double/%d" % n] = (len(S), len(out))
    # k P by double-and-add.  Canonical k: both flavours give k P.  k >= r: the careful flavour gives (k mod r) P; the fast
    # one gives that or a degenerate record (which its callers redo carefully).
    pts = base_points(C, 48)[:8]
    ks = scalar_list(C, rnd)
    rows = [flat(affine_rec(C, pt)) + words_i32(k) for pt in pts for k in ks]
    want = [O.g1_mul(pt, k % O.R) if k % O.R else None for pt in pts for k in ks]
    canon = [k < O.R for pt in pts for k in ks]
    outf = np.asarray(run("g1_29_scalar_mul_fast", _arr(rows))).tolist()
    outc = np.asarray(run("g1_29_scalar_mul_careful", _arr(rows))).tolist()
    dg = np.asarray(run("xyzz29_is_degenerate", _arr([r for r in outf])))[:, 0]
    for i, (rf, rc, w) in enumerate(zip(outf, outc, want)):
        gf, gc = unflat(rf, 4), unflat(rc, 4)
        what = "%s scalar_mul case %d" % (C.name, i)
        assert point_of_xyzz(C, gc) == w and (w is not None or _limbs_zero(gc[2])), what + " (careful)"
        if canon[i] and w is not None:
            assert gf == gc, what + ": fast and careful differ on a canonical scalar"
        else:
            assert dg[i] or point_of_xyzz(C, gf) == w, what + " (fast)"
    count["g1_29_scalar_mul"] = (len(rows), len(outf))
    for op, (g, c) in count.items():
        assert g == c, op
    return count


# ---------------------------------------------------------------- section 4: the pairing decider's lane arithmetic (BN254)
# The pieces of csrc/pairing_coop29.h, decide_w.h, g2_prepare_w.h and the two squeezes of fq29.h / decide_w.h as raw
# records (tests/hosttest/curve_ops.h SNARKV_RAW_DECIDER_OPS), over the operand sets their PRODUCERS can emit.
#
# The sets, in units of p (rho = p / 2^261 = 1 / 169.3 for BN254; "product" = a b / 2^261 + [0, p)):
#   SQUEEZED  what wt_squeeze / fq29_reduce_small (coop3_finalize) leave.  The quotient is round(v8 / p8) of the top limbs
#             (p8 = p >> 232 = 2^21.6) in ONE rounding (a fused multiply-add).  x / p - v8 / p8 = L / p - (v8 / p8)(Lp / p)
#             with L < 7 * 2^232 the lower limbs of a six-term sum and Lp < 2^232 those of p: below 71 * 2^-21.6 = 2.3e-5
#             for |x| <= 64 p; the float path adds |q| 2^-23 + half an ulp of 64 = 1.2e-5.  So |result| <= (1/2 + 2^-13) p.
#   PLAIN_W   a plain value of the program form (k_decide_w): SQUEEZED, the single products of wt_eval_line and wt_fq2inv
#             (a value within 1.01 p times a canonical one: (-0.006 p, 1.006 p); seen for wt_fq2inv: 1.0031 p), the
#             negated product of wt_fq2inv ((-1.006 p, 0.006 p)), canonical constants
#             and key coefficients: inside (-1.01 p, 1.01 p), carry-normalised.
#   XI_W      wt_xi of two PLAIN_W values: 9 own -/+ other, inside (-10.1 p, 10.1 p), carry-normalised.
#   STORED    a coefficient of k_decide's registers: SQUEEZED (coop3_finalize), the canonical start values, and what
#             coop_frob / coop_scale / coop_conj store WITHOUT a squeeze: fq2_scale_norm is a sum (e = 1) or difference
#             (e = 0) of two single products of a STORED value by a value within 1.01 p, i.e. inside
#             (-2.05 / 169.3 - 1, 2 + 2 * 2.05 / 169.3) = (-1.025 p, 2.025 p), and coop_conj negates that: inside
#             (-2.05 p, 2.05 p), carry-normalised: the proven set (seen: -0.993 p .. 1.999 p).  (The headers used to say 1.5 p.)
#   PRODUCT   the fused two-product step over any of these: k_decide multiplies STORED by STORED
#             (2 * 2.05^2 / 169.3 = 0.050), k_decide_w PLAIN_W by PLAIN_W or XI_W (2 * 1.01 * 10.1 / 169.3 = 0.1205): inside
#             (-p/8, 9p/8), carry-normalised.  Six of them sum to (-0.75 p, 6.75 p); low + 9 high +- high' of k + 1 and
#             5 - k of them to (-11.4 p, 57.4 p) (-91/8 and 459/8 at k = 0; both ends are among the records): inside the +-64 p of the squeeze, top limb far inside int32.
from fractions import Fraction

DECIDER_OPS = {
    "fq29_reduce_small": (9, 9), "fq29_mul_small_norm": (10, 9), "wt_squeeze": (9, 9), "wt_xi_e0": (18, 9), "wt_xi_e1": (18, 9),
    "wt_cneg": (10, 9), "coop3_product_e0": (36, 9), "coop3_product_e1": (36, 9), "coop3_finalize_e0": (27, 9),
    "coop3_finalize_e1": (27, 9), "g2w_product_e0": (36, 18), "g2w_product_e1": (36, 18), "fq2_scale_norm_e0": (36, 9),
    "fq2_scale_norm_e1": (36, 9), "wt_fq2inv": (18, 18),
}
ROUND_OPS = {"wt_round": (48 * 9 + 2, 24 * 9), "coop3_round": (24 * 9 + 1, 12 * 9)}
ALL_OPS = dict(OPS, **DECIDER_OPS, **ROUND_OPS)
FLOAT_QUOTIENT_OPS = ("fq29_reduce_small", "wt_squeeze", "coop3_finalize_e0", "coop3_finalize_e1")

SQUEEZED = Fraction(1, 2) + Fraction(1, 1 << 13)
PLAIN_W = Fraction(101, 100)
XI_W = 10 * PLAIN_W
STORED = Fraction(205, 100)
PROD_LO, PROD_HI = Fraction(-1, 8), Fraction(9, 8)
REDUCE_DOMAIN = 64
# the largest |g2w_comb| that interval arithmetic over g2_prepare_prog.inc proves (test_g2_prepare_program_stays_inside_its
# contracts asserts it), rounded up; g2w_product is tested over operands up to it
G2W_COMB_MAX = Fraction(13, 4)
TOP = 1 << 232


def _fr(F, fr):
    """floor(fr * p) as an integer"""
    return (fr.numerator * F.q) // fr.denominator


def residue_classes(F, rnd, n_random):
    q = F.q
    p8 = q >> 232
    edge = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, TOP - 1, TOP, p8 << 232, ((p8 - 1) << 232) | (TOP - 1), F.one]
    return edge + [rnd.randrange(q) for _ in range(n_random)]


def reps(F, res, lo, hi):
    """the smallest and the largest integer of the residue strictly inside (lo, hi), and the canonical one if it is inside"""
    q = F.q
    a = lo + 1 + ((res - lo - 1) % q)
    b = hi - 1 - ((hi - 1 - res) % q)
    return [v for v in (a, b, res) if lo < v < hi]


def value_pool(F, seed, n, lo, hi):
    """n integers strictly inside (lo, hi): every residue class at both ends of the interval and canonical, the ends
    themselves, values whose limbs 0..7 are all ones / all zero at both ends, then seeded random ones"""
    key = (F.q, "vpool", seed, n, lo, hi)
    if key in _CACHE:
        return _CACHE[key]
    rnd = random.Random(seed)
    out = [lo + 1, hi - 1]
    for low in (TOP - 1, 0, (TOP - 1) // 3):
        out += [((lo - low) // TOP + 1) * TOP + low, ((hi - low - 1) // TOP) * TOP + low]
    for r in residue_classes(F, rnd, 12):
        out += reps(F, r, lo, hi)
    out = [v for v in out if lo < v < hi]
    while len(out) < n:
        out.append(rnd.randrange(lo + 1, hi))
    rnd.shuffle(out)
    assert all(lo < v < hi for v in out)
    _CACHE[key] = out[:n]
    return _CACHE[key]


def _sym(F, fr):
    b = _fr(F, fr)
    return -b, b


def _limb_rows(values):
    return np.array([spell(v) for v in values], dtype=np.int64).astype(np.int32)


def vals_u(a):
    """(n, 9) int32 -> integers with limbs 0..7 read as UNSIGNED 32-bit words (a limb-wise sum of up to six), limb 8 signed"""
    a = np.asarray(a)
    out = a[:, 8].astype(object) << 232
    for i in range(8):
        out = out + ((a[:, i].astype(np.int64) & 0xFFFFFFFF).astype(object) << (29 * i))
    return out


def float_quotient(F, top):
    """the quotient estimate of fq29_reduce_small / wt_squeeze: trunc(fma((float) v8, 1.0f / (float) p8, +-0.5f)), bit for
    bit.  The product of two floats is exact in a double and so is its sum with 0.5 once |product| >= 2^-6 (below that the
    result truncates to 0 whatever the rounding), so rounding the double once to float IS the fused operation."""
    top = np.asarray(top, dtype=np.int32)
    inv = np.float32(1.0) / np.float32(F.limbs[8])
    t = top.astype(np.float32).astype(np.float64) * np.float64(inv) + np.where(top >= 0, 0.5, -0.5)
    return t.astype(np.float32).astype(np.int64)


def m_squeeze(F, values, tops):
    """value - q p with the float quotient of the top limb, carry-normalised (limb 8 must fit int32)"""
    return np.array([spell(int(v) - int(k) * F.q) for v, k in zip(values, float_quotient(F, tops))], dtype=np.int64).astype(np.int32)


def _sum_limbs(terms):
    """the limb-wise sum group8_sum leaves: limbs 0..7 below 6 * 2^29 as 32-bit words (int32 view), limb 8 signed"""
    s = [0] * 9
    for t in terms:
        for i, x in enumerate(spell(t)):
            s[i] += x
    assert all(0 <= x < 1 << 32 for x in s[:8])
    return [x - (1 << 32) if i < 8 and x >= I32 else x for i, x in enumerate(s)]


def _split(rnd, total, n, lo, hi):
    """n integers strictly inside (lo, hi) that sum to `total`, or None"""
    if not n * lo + n <= total <= n * hi - n:
        return None
    for _ in range(20):
        base = total // n
        room = min(base - lo, hi - base) // 2
        t = [base + (rnd.randrange(-room, room + 1) if room > 0 else 0) for _ in range(n - 1)]
        t.append(total - sum(t))
        if all(lo < v < hi for v in t):
            return t
    t = [total // n] * (n - 1)
    t.append(total - sum(t))
    return t if all(lo < v < hi for v in t) else None


_HALF_DELTAS = [0, 1, -1, TOP >> 1, -(TOP >> 1), TOP, -TOP, 3 * TOP, -3 * TOP, 7 * TOP, -7 * TOP, 8 * TOP, -8 * TOP]


def _term_extremes(F):
    lo, hi = _fr(F, PROD_LO), _fr(F, PROD_HI) + 1
    ext = [lo + 1, hi - 1]
    for low in (TOP - 1, 0):
        ext += [((lo - low) // TOP + 1) * TOP + low, ((hi - low - 1) // TOP) * TOP + low]
    return lo, hi, ext


def squeeze_cases(F, n):
    """limb-wise sums of 1..6 fused-product outputs for wt_squeeze -> (rows, term lists)"""
    rnd = random.Random(7001)
    q = F.q
    lo, hi, ext = _term_extremes(F)
    pool = value_pool(F, 7002, 4000, lo, hi)
    sums = []
    for nt in range(1, 7):  # the corners: every term at the same extreme, and the extremes alternating
        for e in ext:
            sums.append([e] * nt)
        for e in ext:
            for f in ext:
                sums.append([e if i % 2 == 0 else f for i in range(nt)])
    for res in residue_classes(F, rnd, 40):  # every residue class with the other terms at an extreme
        for nt in range(1, 7):
            for e in ext:
                r = (res - (nt - 1) * e) % q
                for last in (r, r + q, r - q):
                    if lo < last < hi:
                        sums.append([e] * (nt - 1) + [last])
    for k in range(-1, 7):  # totals next to (k + 1/2) p, on both sides
        for d in _HALF_DELTAS + [q >> 18, -(q >> 18), q >> 21, -(q >> 21)]:
            total = ((2 * k + 1) * q) // 2 + d
            for nt in range(1, 7):
                for _ in range(3):
                    t = _split(rnd, total, nt, lo, hi)
                    if t:
                        sums.append(t)
    while len(sums) < n:
        nt = rnd.randrange(1, 7)
        sums.append([rnd.choice(pool) if rnd.random() < 0.7 else rnd.choice(ext) for _ in range(nt)])
    rows = np.array([_sum_limbs(t) for t in sums], dtype=np.int64).astype(np.int32)
    assert (rows[:, :8] < 0).any(), "no limb reached 2^31: the unsigned reading is not exercised"
    assert rows[:, :8].astype(np.int64).__and__(0xFFFFFFFF).max() >= 6 * MASK - 8
    assert rows[:, 8].min() < 0 and rows[:, 8].max() >= 6 * ((hi - 1) >> 232) - 1
    return rows


def finalize_cases(F, n, e):
    """(lo, hi, hp) for coop3_finalize: sums of k + 1, 5 - k and 5 - k fused-product outputs, k = 0..5"""
    rnd = random.Random(7100 + e)
    q = F.q
    lo, hi, ext = _term_extremes(F)
    pool = value_pool(F, 7002, 4000, lo, hi)
    recs = []
    sg = 1 if e else -1
    for k in range(6):
        nl, nh = k + 1, 5 - k
        for a in ext:  # every combination of extremes: this holds the maximum and the minimum of lo + 9 hi +- hp
            for b in ext:
                for c in ext:
                    recs.append(([a] * nl, [b] * nh, [c] * nh))
        for res in residue_classes(F, rnd, 12):  # every residue class at both ends
            for b, c in ((ext[1], ext[1] if e else ext[0]), (ext[0], ext[0] if e else ext[1]), (ext[3], ext[2]), (ext[5], ext[4])):
                for a in (ext[0], ext[1]):
                    r = (res - (nl - 1) * a - 9 * nh * b - sg * nh * c) % q
                    for last in (r, r + q, r - q):
                        if lo < last < hi:
                            recs.append(([a] * (nl - 1) + [last], [b] * nh, [c] * nh))
        for d in _HALF_DELTAS + [q >> 18, -(q >> 18)]:  # lo + 9 hi +- hp next to a half-integer multiple of p
            for _ in range(12):
                th = [rnd.choice(pool) if rnd.random() < 0.6 else rnd.choice(ext) for _ in range(nh)]
                tp = [rnd.choice(pool) if rnd.random() < 0.6 else rnd.choice(ext) for _ in range(nh)]
                base = 9 * sum(th) + sg * sum(tp)
                # integers m with  (m + 1/2) p + d - base  a feasible sum of nl terms
                mlo = -((-(2 * (base + nl * lo - d) + q)) // (2 * q)) + 1
                mhi = (2 * (base + nl * hi - d) - q) // (2 * q) - 1
                if mlo > mhi:
                    continue
                m = rnd.randrange(mlo, mhi + 1)
                tl = _split(rnd, ((2 * m + 1) * q) // 2 + d - base, nl, lo, hi)
                if tl:
                    recs.append((tl, th, tp))
    while len(recs) < n:
        k = rnd.randrange(6)
        pick = lambda m: [rnd.choice(pool) if rnd.random() < 0.7 else rnd.choice(ext) for _ in range(m)]  # noqa: E731
        recs.append((pick(k + 1), pick(5 - k), pick(5 - k)))
    rows = np.array([_sum_limbs(a) + _sum_limbs(b) + _sum_limbs(c) for a, b, c in recs], dtype=np.int64).astype(np.int32)
    top = (hi - 1) >> 232
    for j, nt in ((0, 6), (1, 5), (2, 5)):  # the low block sums up to six terms, the two high blocks up to five
        blk = rows[:, 9 * j:9 * j + 9]
        assert (blk[:, :8] < 0).any(), "block %d: no limb reached 2^31: the unsigned reading is not exercised" % j
        assert blk[:, :8].astype(np.int64).__and__(0xFFFFFFFF).max() >= nt * MASK - 8, j
        assert blk[:, 8].min() < 0 and blk[:, 8].max() >= nt * top - 1, j
    return rows


def reduce_small_cases(F, n):
    """carry-normalised x inside (-64 p, 64 p): every residue class at every multiple of p, and top limbs next to
    (k + 1/2) p8 with the lower limbs all zero, all ones and random"""
    rnd = random.Random(7200)
    q = F.q
    p8 = q >> 232
    vs = []
    res = residue_classes(F, rnd, 8)
    for r in res:
        for k in range(-REDUCE_DOMAIN, REDUCE_DOMAIN):
            vs.append(r + k * q)
    for k in range(-REDUCE_DOMAIN, REDUCE_DOMAIN - 1):
        half = ((2 * k + 1) * q) // 2
        for d in _HALF_DELTAS + [q >> 18, -(q >> 18)]:
            vs.append(half + d)
        t8 = ((2 * k + 1) * p8) // 2
        for d8 in range(-3, 4):
            for low in (0, TOP - 1, rnd.randrange(TOP)):
                vs.append(((t8 + d8) << 232) + low)
    vs = [v for v in vs if -REDUCE_DOMAIN * q < v < REDUCE_DOMAIN * q]
    while len(vs) < n:
        vs.append(rnd.randrange(-REDUCE_DOMAIN * q + 1, REDUCE_DOMAIN * q))
    return _limb_rows(vs)


def _pick(rnd, *pools):
    return rnd.choice(rnd.choice(pools))


def decider_cases(F, n=20000):
    """op -> (>= n, words in) int32 records, every one inside the domain its producers can emit (asserted)"""
    key = (F.q, "decider", n)
    if key in _CACHE:
        return _CACHE[key]
    rnd = random.Random(7300)
    q = F.q
    cases = {}
    plain = value_pool(F, 7301, n, *_sym(F, PLAIN_W))
    plain2 = value_pool(F, 7302, n, *_sym(F, PLAIN_W))
    xi = value_pool(F, 7303, n, *_sym(F, XI_W))
    xi2 = value_pool(F, 7304, n, *_sym(F, XI_W))
    st = [value_pool(F, 7310 + i, n, *_sym(F, STORED)) for i in range(4)]
    canon = value_pool(F, 7320, n, -1, q)
    canon2 = value_pool(F, 7321, n, -1, q)
    comb = [value_pool(F, 7330 + i, n, *_sym(F, G2W_COMB_MAX)) for i in range(4)]
    cases["fq29_reduce_small"] = reduce_small_cases(F, n)
    cases["wt_squeeze"] = squeeze_cases(F, n)
    cases["coop3_finalize_e0"] = finalize_cases(F, n, 0)
    cases["coop3_finalize_e1"] = finalize_cases(F, n, 1)
    two = np.concatenate([_limb_rows(plain), _limb_rows(plain2)], axis=1)
    cases["wt_xi_e0"] = two
    cases["wt_xi_e1"] = two
    m = np.array([[0 if i % 2 else -1] for i in range(n)], dtype=np.int32)
    cn = _limb_rows(plain)
    lazy = _pool(F, 3, n, "lazy")  # any |limb| <= 2^29 works limb-wise
    cases["wt_cneg"] = np.concatenate([np.concatenate([cn[:n // 2], lazy[n // 2:n]]), m], axis=1)
    # fused products: STORED x STORED (k_decide), PLAIN_W x (PLAIN_W | XI_W) (k_decide_w)
    h = n // 2
    a0 = _limb_rows(st[0][:h] + plain[h:])
    a1 = _limb_rows(st[1][:h] + plain2[h:])
    y0 = _limb_rows(st[2][:h] + xi[h:])
    y1 = _limb_rows(st[3][:h] + xi2[h:])
    cases["coop3_product_e0"] = np.concatenate([a0, a1, y0, y1], axis=1)
    cases["coop3_product_e1"] = cases["coop3_product_e0"]
    g = np.concatenate([_limb_rows(c) for c in comb], axis=1)
    cases["g2w_product_e0"] = g
    cases["g2w_product_e1"] = g
    # coop_frob: (stored, stored, gamma, gamma), gamma canonical, and for odd k the y it passes is fq29_neg of the stored
    # one, NOT normalised (limbs in (-2^29, 0], top limb negated): every fourth record, across both kinds of g1; coop_scale: the scalar 1 / d of coop_inv: scal[0] a single
    # product of a squeezed value by a canonical one, scal[1] the limb-wise negation of one (limbs <= 0)
    s0 = value_pool(F, 7340, n, -q // 128, q + q // 128)
    s1 = np.concatenate([_limb_rows(canon2[:h]), -_limb_rows(value_pool(F, 7341, n, -q // 128, q + q // 128)[h:])])
    g0 = _limb_rows(canon[:h] + s0[h:])
    y = _limb_rows(st[1])
    y[1::4] = -y[1::4]
    assert (y[1::4, :8] <= 0).all() and (y[1::4, :8] < 0).any() and (np.abs(y.astype(np.int64)) < (1 << 29)).all()
    cases["fq2_scale_norm_e0"] = np.concatenate([_limb_rows(st[0]), y, g0, s1], axis=1)
    cases["fq2_scale_norm_e1"] = cases["fq2_scale_norm_e0"]
    # wt_fq2inv: d = coefficient 0 of a register a round wrote (SQUEEZED; tested over all of PLAIN_W), d = 0 included
    d = np.concatenate([_limb_rows(plain2), _limb_rows(plain)], axis=1)
    d[0] = 0
    cases["wt_fq2inv"] = d
    # k x: limb 8 of the result must fit int32, i.e. |k| (|x| / 2^232 + 1) < 2^31
    wide = value_pool(F, 7350, n, -8 * q, 8 * q)
    rows = []
    for i in range(n):
        v = wide[i] if i % 3 else plain[i]
        if i % 7 == 0:
            v = rnd.choice([0, 1, -1, TOP - 1, -TOP])
        kmax = min((1 << 20) - 1, (I32 - 1) // ((abs(v) >> 232) + 2))
        k = rnd.choice([kmax, -kmax, 1, -1, 0, 9, -9, rnd.randrange(-kmax, kmax + 1)])
        rows.append(spell(v) + [k])
    cases["fq29_mul_small_norm"] = np.array(rows, dtype=np.int64).astype(np.int32)
    for name, arr in cases.items():
        assert arr.shape[1] == DECIDER_OPS[name][0] and len(arr) >= n, name
    _CACHE[key] = cases
    return cases


def _span(mx, name, values, q):
    lo, hi = min(values), max(values)
    old = mx.get(name, (0.0, 0.0))
    mx[name] = (min(old[0], float(Fraction(int(lo), q))), max(old[1], float(Fraction(int(hi), q))))


def _assert_norm(out, what):
    out = np.asarray(out)
    assert ((out[:, :8] >= 0) & (out[:, :8] <= MASK)).all(), what + ": a limb 0..7 outside [0, 2^29)"


def _assert_within(values, lo, hi, q, what):
    bad = [i for i, v in enumerate(values) if not lo <= v <= hi]
    assert not bad, "%s: %d values outside [%.4f p, %.4f p], first at %d: %.6f p" % (
        what, len(bad), lo / q, hi / q, bad[0], values[bad[0]] / q)


def decider_suite(F, run, n=20000):
    """Every decider piece over `decider_cases` through `run(op, in) -> out`; each record against exact integers: residue,
    limbs 0..7 in [0, 2^29), the set the consumers rely on, and (where the model fixes them) the nine limbs.
    Returns ({op: records checked}, {bound name: (smallest, largest value / p seen)})."""
    q = F.q
    cases = decider_cases(F, n)
    outs = {name: np.asarray(run(name, inp)) for name, inp in cases.items()}
    checked, mx = {}, {}
    sq = _fr(F, SQUEEZED)
    # ---- the two float-quotient squeezes and the finalisation built on one
    inp = cases["fq29_reduce_small"]
    assert ((inp[:, :8] >= 0) & (inp[:, :8] <= MASK)).all()
    x = vals(inp)
    for name, x, top in (("fq29_reduce_small", x, inp[:, 8]), ("wt_squeeze", vals_u(cases["wt_squeeze"]), cases["wt_squeeze"][:, 8])):
        o = outs[name]
        _assert_norm(o, name)
        v = vals(o)
        assert all((a - b) % q == 0 for a, b in zip(v, x)), name + ": residue changed"
        _assert_within(v, -sq, sq, q, name)
        checked[name] = _eq(o, m_squeeze(F, x, top), name + " against the model's quotient")
        _span(mx, name, v, q)
    for e in (0, 1):
        name = "coop3_finalize_e%d" % e
        inp = cases[name]
        lo, hi, hp = vals_u(inp[:, :9]), vals_u(inp[:, 9:18]), vals_u(inp[:, 18:])
        t = lo + 9 * hi + (hp if e else -hp)
        assert all(-REDUCE_DOMAIN * q < v < REDUCE_DOMAIN * q for v in t)
        _span(mx, "coop3_finalize input", t, q)
        o = outs[name]
        _assert_norm(o, name)
        v = vals(o)
        assert all((a - b) % q == 0 for a, b in zip(v, t)), name + ": residue is not lo + 9 hi +- hp"
        _assert_within(v, -sq, sq, q, name)
        tops = np.array([spell(int(z))[8] for z in t], dtype=np.int64).astype(np.int32)
        checked[name] = _eq(o, m_squeeze(F, t, tops), name + " against the model's quotient")
        _span(mx, "coop3_finalize", v, q)
    # ---- xi copies: the exact integer 9 own -/+ other, inside the bound the products need
    xb = _fr(F, XI_W)
    for e in (0, 1):
        name = "wt_xi_e%d" % e
        inp = cases[name]
        own, other = vals(inp[:, :9]), vals(inp[:, 9:])
        want = 9 * own + (other if e else -other)
        o = outs[name]
        _assert_norm(o, name)
        assert (vals(o) == want).all(), name + ": not the integer 9 own %s other" % ("+" if e else "-")
        _assert_within(want, -xb, xb, q, name)
        checked[name] = len(o)
        _span(mx, "wt_xi", want, q)
    inp = cases["wt_cneg"]
    want = np.where(inp[:, 9:10] != 0, -inp[:, :9], inp[:, :9])
    checked["wt_cneg"] = _eq(outs["wt_cneg"], want, "wt_cneg")
    # ---- fused two-product steps
    plo, phi = _fr(F, PROD_LO), _fr(F, PROD_HI)
    for e in (0, 1):
        name = "coop3_product_e%d" % e
        inp = cases[name]
        assert (np.abs(inp.astype(np.int64)) < (1 << 29)).all()
        a0, a1, y0, y1 = (vals(inp[:, 9 * j:9 * j + 9]) for j in range(4))
        t = a0 * y0 + (a1 * y1 if e else -(a1 * y1))
        checked[name] = check_product(F, outs[name], t, name)
        exp = np.array([spell((z + ((z * F.nqinv) % F.R) * q) >> RBITS) for z in t], dtype=np.int64).astype(np.int32)
        _eq(outs[name], exp, name + " against the closed form")
        v = vals(outs[name])
        _assert_within(v, plo + 1, phi, q, name)
        _span(mx, "fused product", v, q)
        name = "g2w_product_e%d" % e
        inp = cases[name]
        am, bm, ap, bp = (vals(inp[:, 9 * j:9 * j + 9]) for j in range(4))
        t = ap * bm + am * bp if e else am * bm - ap * bp
        o = outs[name]
        checked[name] = check_product(F, o[:, :9], t, name)
        v = vals(o[:, :9])
        _assert_within(v, -q + 1, 2 * q - 1, q, name + " (the contract of fq29_canon_of_product)")
        _span(mx, "g2w product", v, q)
        _eq(o[:, 9:], _canon_expect(F, o[:, :9]), name + ": the line coefficient is not the canonical representative")
    # ---- what coop_frob / coop_scale store
    sb = _fr(F, STORED)
    for e in (0, 1):
        name = "fq2_scale_norm_e%d" % e
        inp = cases[name].tolist()
        exp = []
        for r in inp:
            x, y, g0, g1 = r[:9], r[9:18], r[18:27], r[27:]
            exp.append(l_norm(l_add(m_mul(F, x, g1), m_mul(F, y, g0)) if e else l_sub(m_mul(F, x, g0), m_mul(F, y, g1))))
        o = outs[name]
        _assert_norm(o, name)
        checked[name] = _eq(o, np.array(exp, dtype=np.int64).astype(np.int32), name + " against the model")
        v = vals(o)
        x, y, g0, g1 = (vals(cases[name][:, 9 * j:9 * j + 9]) for j in range(4))
        t = x * g1 + y * g0 if e else x * g0 - y * g1
        assert all((a * F.R - b) % q == 0 for a, b in zip(v, t)), name + ": residue"
        _assert_within(v, -sb, sb, q, name + " (the stored-coefficient set)")
        _span(mx, "fq2_scale_norm", v, q)
    # ---- WT_FQ2INV's lane: (d0 - d1 u) / (d0^2 + d1^2) in the Montgomery form, both values PLAIN_W
    inp = cases["wt_fq2inv"]
    o = outs["wt_fq2inv"]
    d0, d1 = vals(inp[:, :9]), vals(inp[:, 9:])
    v0, v1 = vals(o[:, :9]), vals(o[:, 9:])
    _assert_norm(o[:, :9], "wt_fq2inv")
    _assert_norm(o[:, 9:], "wt_fq2inv")
    r2 = F.R * F.R % q
    for a0, a1, b0, b1 in zip(d0, d1, v0, v1):
        nn = (a0 * a0 + a1 * a1) % q
        assert (b0 * nn - a0 * r2) % q == 0 and (b1 * nn + a1 * r2) % q == 0, "wt_fq2inv: not conj(d) / norm(d)"
        assert nn or (b0 % q == 0 and b1 % q == 0)
    pw = _fr(F, PLAIN_W)
    _assert_within(list(v0) + list(v1), -pw, pw, q, "wt_fq2inv (a plain value of the program form)")
    checked["wt_fq2inv"] = len(o)
    _span(mx, "wt_fq2inv", list(v0) + list(v1), q)
    inp = cases["fq29_mul_small_norm"]
    want = vals(inp[:, :9]) * inp[:, 9].astype(object)
    o = outs["fq29_mul_small_norm"]
    _assert_norm(o, "fq29_mul_small_norm")
    assert (vals(o) == want).all(), "fq29_mul_small_norm: not k x"
    checked["fq29_mul_small_norm"] = len(o)
    for name in cases:
        assert checked[name] == len(cases[name]) >= n, name
    return checked, mx


# ---------------------------------------------------------------- section 4b: whole rounds on raw records
WT_MUL, WT_PW, WT_FQ2INV = 1, 2, 3
WT_A_LINE, WT_B_LINE, WT_A_CONJ, WT_B_CONJ, WT_A_UCONJ, WT_B_BCAST = 1, 2, 4, 8, 16, 32
# every (kind, flags) wt_build_program() emits (the host hook hc_wt_variants lists them; the test compares); WT_FQ2INV is
# one lane's wt_fq2inv, not a round of the duo: the raw operation wt_fq2inv of section 4 covers it
WT_VARIANTS = [(WT_MUL, 0), (WT_MUL, WT_A_LINE | WT_B_LINE), (WT_MUL, WT_A_CONJ), (WT_MUL, WT_B_CONJ),
               (WT_PW, 0), (WT_PW, WT_A_UCONJ), (WT_PW, WT_B_BCAST)]
_PATTERNS = ("max", "min", "alt_e", "alt_k", "alt_ek", "canon", "rand")
_POISON = [MASK] * 8 + [0x5A5A5A]  # an operand slot the operation must not read


def fq12_operand(F, rnd, bound, pattern):
    """12 integers strictly inside (-bound, bound), coefficient c = 2 k + e <-> u^e w^k: residues from the corner classes,
    each at the end of the interval the sign pattern asks for"""
    res = residue_classes(F, rnd, 6)
    out = []
    for c in range(12):
        r = rnd.choice(res)
        rp = reps(F, r, -bound, bound)
        small, large = rp[0], rp[1]
        k, e = c >> 1, c & 1
        up = {"max": True, "min": False, "alt_e": e == 0, "alt_k": k % 2 == 0, "alt_ek": (k + e) % 2 == 0,
              "canon": None, "rand": rnd.random() < 0.5}[pattern]
        out.append(r if up is None else large if up else small)
    return out


def _fq12_of(coef):
    O = BN
    f = [O.Fq2(coef[2 * i], coef[2 * i + 1]) for i in range(6)]
    return O.Fq12(O.Fq6(f[0], f[2], f[4]), O.Fq6(f[1], f[3], f[5]))


def _flat_of(x):
    c6 = [x.c0.c0, x.c1.c0, x.c0.c1, x.c1.c1, x.c0.c2, x.c1.c2]  # w^0 .. w^5
    return [v for f in c6 for v in (f.a, f.b)]


def _conj_flat(coef):
    return [-v if (c >> 1) & 1 else v for c, v in enumerate(coef)]


def _with_xi(coef):
    """plain coefficients followed by their xi copies (component e of xi * (c0 + c1 u))"""
    out = list(coef)
    for i in range(len(coef) // 2):
        c0, c1 = coef[2 * i], coef[2 * i + 1]
        out += [9 * c0 - c1, c0 + 9 * c1]
    return out


def wt_round_cases(F, per_variant=2000):
    """records of k_wt_round for every variant -> (rows, [(kind, flags, expected 12 residues times 2^261)])"""
    key = (F.q, "wt_round", per_variant)
    if key in _CACHE:
        return _CACHE[key]
    rnd = random.Random(7400)
    q = F.q
    bound = _fr(F, PLAIN_W)
    rows, meta = [], []
    for kind, flags in WT_VARIANTS:
        for i in range(per_variant):
            pa, pb = _PATTERNS[i % 7], _PATTERNS[(i // 7) % 7]
            A = fq12_operand(F, rnd, bound, pa)
            B = A if (i % 11 == 0 and not flags & (WT_A_LINE | WT_B_LINE | WT_B_BCAST)) else fq12_operand(F, rnd, bound, pb)
            if i % 13 == 0:  # a sparse B
                B = [v if (c >> 1) in (0, 1, 3) else 0 for c, v in enumerate(B)]
            la = [0, 1, 2, 3, 6, 7]  # the coefficients of w^0, w^1, w^3
            if kind == WT_MUL:
                if flags & WT_A_LINE:
                    A = [v if c in la else 0 for c, v in enumerate(A)]
                    areg = [spell(A[c]) for c in la] + [_POISON] * 18
                else:
                    areg = [spell(v) for v in _with_xi(A)]
                if flags & WT_B_LINE:
                    B = [v if c in la else 0 for c, v in enumerate(B)]
                    breg = [spell(v) for v in _with_xi([B[c] for c in la])] + [_POISON] * 12
                else:
                    breg = [spell(v) for v in _with_xi(B)]
                ea = _conj_flat(A) if flags & WT_A_CONJ else A
                eb = _conj_flat(B) if flags & WT_B_CONJ else B
                exp = _flat_of(_fq12_of(ea) * _fq12_of(eb))
            else:
                areg = [spell(v) for v in _with_xi(A)]
                if flags & WT_B_BCAST:
                    breg = [spell(B[0]), spell(B[1])] + [_POISON] * 22
                else:
                    breg = [spell(v) for v in B] + [_POISON] * 12
                exp = []
                for k in range(6):
                    a = BN.Fq2(A[2 * k], A[2 * k + 1])
                    if flags & WT_A_UCONJ:
                        a = a.conj()
                    if (flags & WT_A_CONJ) and k & 1:
                        a = -a
                    j = 0 if flags & WT_B_BCAST else k
                    r = a * BN.Fq2(B[2 * j], B[2 * j + 1])
                    exp += [r.a, r.b]
            rows.append(flat(areg, breg) + [kind, flags])
            meta.append((kind, flags, exp))
    out = (np.array(rows, dtype=np.int64).astype(np.int32), meta)
    _CACHE[key] = out
    return out


def check_wt_round(F, out, meta):
    """a round's 24 stored values: the product's residues, the stored-coefficient invariant, the exact xi copies"""
    q = F.q
    sq = _fr(F, SQUEEZED)
    out = np.asarray(out)
    assert out.shape == (len(meta), 24 * 9)
    _assert_norm(out.reshape(-1, 9), "wt_round")
    v = vals(out.reshape(-1, 9)).reshape(len(meta), 24)
    count = {}
    for i, (kind, flags, exp) in enumerate(meta):
        row = v[i]
        for c in range(12):
            assert (row[c] * F.R - exp[c]) % q == 0, "wt_round record %d (kind %d flags %d): coefficient %d" % (i, kind, flags, c)
            assert -sq <= row[c] <= sq, "wt_round record %d: coefficient %d at %.5f p" % (i, c, row[c] / q)
        for k in range(6):
            c0, c1 = row[2 * k], row[2 * k + 1]
            assert row[12 + 2 * k] == 9 * c0 - c1 and row[13 + 2 * k] == c0 + 9 * c1, "wt_round record %d: xi copy of w^%d" % (i, k)
        count[(kind, flags)] = count.get((kind, flags), 0) + 1
    return count, (float(Fraction(int(v[:, :12].min()), q)), float(Fraction(int(v[:, :12].max()), q)))


def coop3_round_cases(F, n=2000):
    """records of k_coop3_round: dense B, sparse / line-shaped B (mode 1, the unread coefficients poisoned), A == B"""
    key = (F.q, "coop3_round", n)
    if key in _CACHE:
        return _CACHE[key]
    rnd = random.Random(7500)
    bound = _fr(F, STORED)
    rows, meta = [], []
    for mode in (0, 1):
        for i in range(n):
            A = fq12_operand(F, rnd, bound, _PATTERNS[i % 7])
            B = A if (mode == 0 and i % 11 == 0) else fq12_operand(F, rnd, bound, _PATTERNS[(i // 7) % 7])
            if mode == 1 or i % 13 == 0:
                B = [v if (c >> 1) in (0, 1, 3) else 0 for c, v in enumerate(B)]
            exp = _flat_of(_fq12_of(A) * _fq12_of(B))
            bl = [spell(v) if (mode == 0 or (c >> 1) in (0, 1, 3)) else _POISON for c, v in enumerate(B)]
            rows.append(flat([spell(v) for v in A], bl) + [mode])
            meta.append((mode, 0, exp))
    out = (np.array(rows, dtype=np.int64).astype(np.int32), meta)
    _CACHE[key] = out
    return out


def check_coop3_round(F, out, meta):
    q = F.q
    sq = _fr(F, SQUEEZED)
    out = np.asarray(out)
    assert out.shape == (len(meta), 12 * 9)
    _assert_norm(out.reshape(-1, 9), "coop3_round")
    v = vals(out.reshape(-1, 9)).reshape(len(meta), 12)
    for i, (mode, _, exp) in enumerate(meta):
        for c in range(12):
            assert (v[i][c] * F.R - exp[c]) % q == 0, "coop3_round record %d (mode %d): coefficient %d" % (i, mode, c)
            assert -sq <= v[i][c] <= sq, "coop3_round record %d: coefficient %d at %.5f p" % (i, c, v[i][c] / q)
    return len(meta), (float(Fraction(int(v.min()), q)), float(Fraction(int(v.max()), q)))


# ---------------------------------------------------------------- section 4c: the level program of k_g2_prepare_w
def g2w_program(lib):
    """kG2wProg as the host build holds it: (levels, tasks, start slots, [[task dict] per level]); the start slots are
    the program's own constants (hc_g2w_slot): ([canonical at the start], [zero at the start])"""
    import ctypes

    levels, tasks, nslots = (lib.hc_g2w_dims(i) for i in range(3))
    named = [lib.hc_g2w_slot(i) for i in range(12)]  # ONE B3 G12 G13 G22 G23, QX QY, TX TZ TYA, TYB
    assert lib.hc_g2w_slot(12) == -1 and len(set(named)) == 12 and all(0 <= s < nslots for s in named)
    slots = (named[:11], named[11:])  # k_g2_prepare_w starts T at (QX, 1, QY) with TYB = 0
    buf = (ctypes.c_int32 * (16 * levels * tasks))()
    assert lib.hc_g2w_prog(buf, levels * tasks) == levels * tasks
    prog = []
    for lv in range(levels):
        row = []
        for t in range(tasks):
            o = list(buf[16 * (lv * tasks + t):16 * (lv * tasks + t) + 16])
            row.append({"dst": o[0], "out": o[1], "as": o[2:5], "ac": o[5:8], "bs": o[8:11], "bc": o[11:14], "conj": o[14], "used": o[15]})
        prog.append(row)
    return levels, tasks, slots, prog


_IV = 1 << 48  # intervals are integers in units of p / 2^48, rounded outward at every product


def _imul(a, b):
    c = [a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]]
    return min(c), max(c)


def g2w_intervals(F, prog, slots):
    """Intervals in units of p through every level (outward-rounded fixed point).  slots = (the constants, Q and the start
    state of T: canonical, [0, 1); the slot that starts at zero), from g2w_program; a combination is sum coeff * slot; a fused-product output is (a b + c d) p / 2^261 + [0, 1).
    Returns (largest |combination|, (smallest, largest) value handed to fq29_canon_of_product, problems found)."""
    zero, canon = (0, 0), (0, _IV)
    sl = {s: [canon, canon] for s in slots[0]}
    sl.update({s: [zero, zero] for s in slots[1]})
    comb_max, line_lo, line_hi, bad = 0, 0, 0, []

    def comb(ss, cs, e, sgn, where):
        lo = hi = 0
        pos = neg = 0
        for s, c in zip(ss, cs):
            c *= sgn
            if c == 0:
                continue
            if s not in sl:
                bad.append("%s reads slot %d before anything wrote it" % (where, s))
                continue
            a, b = sl[s][e]
            lo += min(c * a, c * b)
            hi += max(c * a, c * b)
            pos += max(c, 0)
            neg += max(-c, 0)
        # fq29_norm of the limb-wise sum: every limb of the sum, plus the carry of the one below, must fit int32
        if max(pos, neg) * MASK + 8 >= I32:
            bad.append("%s: a limb of the combination can leave int32" % where)
        return lo, hi

    def scale(lo, hi):  # (units^2 of p^2) -> units of p: times p / 2^261, floor / ceiling, plus [0, 1)
        d = _IV * F.R
        return (lo * F.q) // d, -((-hi * F.q) // d) + _IV

    for lv, row in enumerate(prog):
        written = {t["dst"] for t in row if t["used"] and t["dst"] >= 0}
        new = {}
        for ti, t in enumerate(row):
            if not t["used"]:
                continue
            where = "level %d task %d" % (lv, ti)
            read = {s for s, c in zip(t["as"] + t["bs"], t["ac"] + t["bc"]) if c}
            if read & written:
                bad.append("%s reads slot(s) %s that the same level writes" % (where, sorted(read & written)))
            A = [comb(t["as"], t["ac"], e, -1 if (t["conj"] and e) else 1, where) for e in (0, 1)]
            B = [comb(t["bs"], t["bc"], e, 1, where) for e in (0, 1)]
            for iv in A + B:
                comb_max = max(comb_max, -iv[0], iv[1])
            m00, m11, m01, m10 = _imul(A[0], B[0]), _imul(A[1], B[1]), _imul(A[0], B[1]), _imul(A[1], B[0])
            v0 = scale(m00[0] - m11[1], m00[1] - m11[0])
            v1 = scale(m01[0] + m10[0], m01[1] + m10[1])
            if t["dst"] >= 0:
                new[t["dst"]] = [v0, v1]
            else:
                line_lo, line_hi = min(line_lo, v0[0], v1[0]), max(line_hi, v0[1], v1[1])
        sl.update(new)
    return Fraction(comb_max, _IV), (Fraction(line_lo, _IV), Fraction(line_hi, _IV)), bad


def mul2_column_peak(F, top_units):
    """the largest column sum of fq29_mul2 over carry-normalised operands (or their limb-wise negations) within
    top_units * p: limbs 0..7 at 2^29 - 1, limb 8 at the value's own top, plus the reduction products and the carry"""
    l = [MASK] * 8 + [int(top_units * F.q) >> 232]
    peak = 0
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        s = 2 * sum(l[i] * l[k - i] for i in range(lo, hi + 1))
        red = MASK * sum(F.limbs[k - i] for i in range(lo, hi + 1))
        peak = max(peak, s + red + (1 << 35))
    return peak


# ---------------------------------------------------------------- the builds
def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def _csrc_files():
    d = os.path.join(ROOT, "snark-verifier_amd", "csrc")
    return [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".h", ".hpp", ".inc"))]


def host_lib(curve):
    """tests/hosttest/hosttest_curve.cpp compiled with g++ (the plain-C bodies), rebuilt when stale"""
    import ctypes
    import subprocess

    d = os.path.join(ROOT, "tests", "hosttest")
    so = os.path.join(d, "libhosttest_%s.so" % curve)
    src = os.path.join(d, "hosttest_curve.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < _newest([src, os.path.join(d, "curve_ops.h")] + _csrc_files()):
        flags = ["-DSNARKV_CURVE_PALLAS"] if curve == "pallas" else []
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.hc_curve.restype = ctypes.c_char_p
    assert lib.hc_curve() == curve.encode()
    return lib


def host_runner(curve):
    import ctypes

    lib = host_lib(curve)
    table = ALL_OPS if curve == "bn254" else OPS  # the decider's pieces and rounds exist for BN254 only
    for op, (wi, wo) in table.items():
        assert getattr(lib, "hc_%s_raw_io" % op)() == (wi << 16) | wo, op  # the table above is the header's

    def run(op, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.ndim == 2 and a.shape[1] == table[op][0], op
        out = np.zeros((len(a), table[op][1]), dtype=np.int32)
        getattr(lib, "hc_%s_raw" % op)(a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), len(a))
        return out

    return run


def load_build():
    """snark-verifier_amd/build.py as a module (the package directory has a dash in its name)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
