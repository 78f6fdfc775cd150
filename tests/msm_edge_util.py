"""Inputs that drive the Pippenger (csrc/msm_pippenger.hip) at the edges of its schedule, for both libraries -- a helper
of the tests, no conftest.  Three things:

  * the launcher's geometry restated (`pip_plan`): window size, level-1 keys, piece cap;
  * a bucket planner (`plan_buckets`): scalars d < 2^15 have the GLV halves (d, 0), so bucket d - 1 of window 0 gets
    exactly the planned entries -- with distinct points, duplicates, opposite points or nothing but copies of +-P --
    and the expected point comes from the plan, not from the code under test;
  * scalars with crafted GLV halves (`crafted_scalars`): windows equal to B = 2^(c-1), B + 1, all ones, and B-chains,
    where the carry of the signed-digit recoding is decided windows further down.

Everything the GPU tests assume about these inputs is checked on the CPU in tests/test_msm_edge_util.py, against a
restatement of the recoders (`for_each_digit`, `digit_of_window`) and the host build of csrc/glv.h."""
import ctypes
import functools
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

# ---- constants of csrc/msm_pippenger.hip (GLV builds: both curves) ----
K_HALVES = 2
DIGIT_BITS = 128          # kDigitBits: a 127-bit half + the recoding carry
K_RUN = 128               # SNARKV_KRUN
K_RUN_THROUGHPUT = 128    # SNARKV_KRUN_THROUGHPUT: the cap under the throughput hint
SORT_CAP = 7168           # kSortCap: items k_sort_level2 sorts inside LDS
SORT_TARGET = 3072        # kSortTarget
MAX_KEYS = 16384          # kMaxKeys
BIG_PIECES = 24           # kBigPieces: split buckets of more pieces go to k_fixup's cooperative list
TILE = 2048               # SNARKV_TILE_BASE


def default_window_bits(n):
    best, best_cost = 2, 0.0
    for c in range(2, 23):
        W = (DIGIT_BITS + c - 1) // c
        top = DIGIT_BITS - 1 - (W - 1) * c
        cost = float(K_HALVES) * float(n) * W * 10.0 + float(W) * float(1 << (c - 1)) * 30.0
        if top < c - 3:
            cost *= 1.6
        if c == 2 or cost < best_cost:
            best, best_cost = c, cost
    return best


def balance_window_bits(c):
    W = (DIGIT_BITS + c - 1) // c
    return (DIGIT_BITS + W - 1) // W


def latency_run_length(entries):
    waves = lambda run: (entries + 64 * run - 1) // (64 * run)  # noqa: E731
    if waves(16) <= 4608:
        return 16 if waves(16) >= 2048 else 32
    if waves(32) <= 4608:
        return 32
    return K_RUN


def pip_plan(n, window_bits=0, hint=False):
    """`launch_msm_pippenger_phases` for an n-term MSM -> (c, W, B, low_bits, SB, cap)"""
    c = window_bits if window_bits > 0 else balance_window_bits(default_window_bits(n))
    c = min(max(c, 2), 22)
    W = (DIGIT_BITS + c - 1) // c
    B = 1 << (c - 1)
    high = c - 1 - 10 if c - 1 > 10 else 0
    while high < c - 1 and ((K_HALVES * n) >> (high + 1)) >= SORT_TARGET and (W << (high + 1)) <= MAX_KEYS:
        high += 1
    low_bits = (c - 1) - high
    cap = K_RUN_THROUGHPUT if hint else latency_run_length(K_HALVES * n * W)
    return c, W, B, low_bits, B >> low_bits, cap


# ---- the digit recoders, restated ----
def for_each_digit(mag, c):
    """`for_each_digit` on one magnitude (< 2^127): [(window, |digit|, negative)] of the non-zero digits"""
    W, B, out, carry = (DIGIT_BITS + c - 1) // c, 1 << (c - 1), [], 0
    for w in range(W):
        raw = ((mag >> (w * c)) & ((1 << c) - 1)) + carry
        neg = 1 if raw > B else 0
        d = (1 << c) - raw if neg else raw
        carry = neg
        if d:
            out.append((w, d, neg))
    return out


def digit_of_window(mag, c, w):
    """`digit_of_window`: the same digit without walking the windows below -- (|digit|, negative), or None for a zero digit"""
    B, carry = 1 << (c - 1), 0
    for j in range(w - 1, -1, -1):
        b = (mag >> (j * c)) & ((1 << c) - 1)
        if b != B:
            carry = 1 if b > B else 0
            break
    raw = ((mag >> (w * c)) & ((1 << c) - 1)) + carry
    neg = 1 if raw > B else 0
    d = (1 << c) - raw if neg else raw
    return (d, neg) if d else None


# ---- the curves ----
class Curve:
    """One library's curve: its oracle module, the host build of its device headers, sampled points as bytes"""

    def __init__(self, name):
        self.name, self.O = name, (PA if name == "pallas" else BN)
        self._lam = None

    @functools.cached_property
    def host(self):
        """tests/hosttest/libhosttest_<curve>.so, as tests/test_curve_math_host.py builds it"""
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("curve", self.name))
        lib.hc_curve.restype = ctypes.c_char_p
        assert lib.hc_curve() == self.name.encode()
        return lib

    def glv_decompose(self, k):
        """csrc/glv.h `glv_decompose` on the host -> the signed halves (k1, k2)"""
        out = ctypes.create_string_buffer(32)
        self.host.hc_glv_decompose(self.O.fe_to_bytes(k), out)
        h = [int.from_bytes(out.raw[:16], "little"), int.from_bytes(out.raw[16:], "little")]
        return tuple(-(v & ((1 << 127) - 1)) if v >> 127 else v for v in h)

    @property
    def lam(self):
        """the cube root of unity mod r that `glv_decompose` maps to the halves (0, 1)"""
        if self._lam is None:
            R = self.O.R
            w = next(x for x in (pow(g, (R - 1) // 3, R) for g in range(2, 40)) if x != 1)
            hits = [x for x in (w, w * w % R) if self.glv_decompose(x) == (0, 1)]
            assert len(hits) == 1
            self._lam = hits[0]
        return self._lam

    def base_bytes(self, nb, seed=0x5EED):
        """nb sampled points as one byte string; pallas has no C oracle and samples ~1 ms per point: one cached set"""
        if self.name == "pallas":
            return b"".join(PA.g1_to_bytes(q) for q in _pallas_base()[:nb])
        import coracle as C

        return C.sample_points(seed, nb)

    def msm(self, scalars, points_bytes, small=False):
        """the plain oracle MSM: integer scalars (mod r), points as bytes -> affine bytes"""
        O = self.O
        n = len(scalars)
        assert n and len(points_bytes) == 64 * n
        if self.name == "bn254":
            import coracle as C

            return C.msm_pippenger(b"".join(O.fe_to_bytes(s % O.R) for s in scalars), points_bytes, 4)
        pts = [O.g1_from_bytes(points_bytes[64 * i:64 * i + 64]) for i in range(n)]
        if small:  # signed scalars of a few dozen bits: |s| on -P, and a window that suits them
            pts = [O.g1_neg(q) if s < 0 else q for s, q in zip(scalars, pts)]
            return O.g1_to_bytes(O.g1_msm_pippenger([abs(s) for s in scalars], pts, 8))
        return O.g1_to_bytes(O.g1_msm_pippenger([s % O.R for s in scalars], pts))

    def mul(self, point_bytes, k):
        O = self.O
        if self.name == "bn254":
            import coracle as C

            return C.g1_mul(point_bytes, O.fe_to_bytes(k % O.R))
        return O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(point_bytes), k))


PALLAS_BASE = 1024  # the cycled base of the pallas tests (the issue's bound is 4096)


@functools.lru_cache(maxsize=None)
def _pallas_base():
    return PA.sample_points(0xBA5E, PALLAS_BASE)


@functools.lru_cache(maxsize=None)
def curve(name):
    return Curve(name)


def _neg_bytes(cv, pb):
    """the points of a byte string negated (the identity does not occur in a base)"""
    P = cv.O.P
    a = np.frombuffer(pb, dtype=np.uint8).reshape(-1, 64).copy()
    for i in range(a.shape[0]):
        y = int.from_bytes(a[i, 32:].tobytes(), "little")
        a[i, 32:] = np.frombuffer(((P - y) % P).to_bytes(32, "little"), dtype=np.uint8)
    return a


def fold_to_base(cv, scalars, nb):
    """MSM of term i = scalars[i] * base[i mod nb], folded on the host to the nb-term oracle MSM of the summed scalars"""
    R = cv.O.R
    coef = [0] * min(nb, len(scalars))
    for i, s in enumerate(scalars):
        coef[i % nb] = (coef[i % nb] + s) % R
    return cv.msm(coef, cv.base_bytes(len(coef)))


# ---- the bucket planner ----
class Plan:
    """scalars / points of a planned MSM: .s, .p (bytes), .n, .digit (d per term), .point (index into the base), .sign
    (+-1), .lengths {d: entries of bucket d - 1 of window 0}, .expected() (affine bytes)"""

    def __init__(self, cv, digit, point, sign, nb):
        self.cv, self.digit, self.point, self.sign, self.nb = cv, digit, point, sign, nb
        self.n = len(digit)
        assert self.n and int(digit.min()) >= 1 and int(digit.max()) < (1 << 15)
        sc = np.zeros((self.n, 32), dtype=np.uint8)
        sc[:, :8] = digit.astype("<u8").view(np.uint8).reshape(self.n, 8)
        self.s = sc.tobytes()
        base = cv.base_bytes(nb)
        pos, neg = np.frombuffer(base, dtype=np.uint8).reshape(nb, 64), _neg_bytes(cv, base)
        self.p = np.where((sign > 0)[:, None], pos[point], neg[point]).tobytes()
        cnt = np.bincount(digit)
        self.lengths = {int(d): int(cnt[d]) for d in np.nonzero(cnt)[0]}

    def expected(self):
        """sum_i +-d_i P_i = sum over the base of (the signed sum of the digits on that point) x the point"""
        coef = np.bincount(self.point, weights=(self.digit * self.sign).astype(np.float64), minlength=self.nb)
        coef = [int(round(v)) for v in coef]  # |sum| < 2^15 n < 2^53: exact in a double
        live = [j for j, v in enumerate(coef) if v]
        if not live:
            return bytes(64)
        base = self.cv.base_bytes(self.nb)
        return self.cv.msm([coef[j] for j in live], b"".join(base[64 * j:64 * j + 64] for j in live), small=True)


def plan_buckets(cv, specs, fill, nb=None):
    """`specs`: planned buckets, spec i -> bucket d - 1 of window 0 with d = 2 i + 3, each (length, kind):
         "distinct"                  `length` different points
         ("marks", [(j, k), ...])    different points, but entry j is a copy (k = "dup") or the negation ("neg") of entry 0
         ("pm", a, b)                nothing but a copies of P and b copies of -P (a + b = length)
       `fill`: the digits d of the remaining terms (any order, none of the planned d), whose points cycle through the
       base.  Asserted: no bucket holds a point twice except where the plan says so."""
    dg, pt, sg, planned, loose = [], [], [], set(), []
    at = 0  # the planned buckets walk the base from here, so that neighbouring buckets do not share their points
    nb = nb or (PALLAS_BASE if cv.name == "pallas" else max(64, min(4096, sum(s[0] for s in specs) + len(fill))))
    for i, (length, kind) in enumerate(specs):
        d = 2 * i + 3
        planned.add(d)
        idx = [(at + j) % nb for j in range(length)]
        sign = [1] * length
        free = [False] * length  # entries that may repeat a point of their bucket
        if kind == "distinct":
            assert length <= nb
        elif kind[0] == "marks":
            assert length <= nb
            for j, k in kind[1]:
                assert 0 < j < length and k in ("dup", "neg")
                idx[j], sign[j], free[j] = idx[0], (1 if k == "dup" else -1), True
        else:
            assert kind[0] == "pm" and kind[1] + kind[2] == length
            idx, sign, free = [at % nb] * length, [1] * kind[1] + [-1] * kind[2], [True] * length
        dg += [d] * length
        pt += idx
        sg += sign
        loose += free
        at += length if kind[0] != "pm" else 1
    fill = np.asarray(fill, dtype=np.int64)
    assert not planned & set(np.unique(fill).tolist())
    digit = np.concatenate([np.asarray(dg, dtype=np.int64), fill])
    point = np.concatenate([np.asarray(pt, dtype=np.int64), np.arange(len(fill), dtype=np.int64) % nb])
    sign = np.concatenate([np.asarray(sg, dtype=np.int64), np.ones(len(fill), dtype=np.int64)])
    strict = np.concatenate([~np.asarray(loose, dtype=bool), np.ones(len(fill), dtype=bool)])
    keys = (digit * nb + point)[strict]
    assert len(np.unique(keys)) == len(keys), "a bucket holds one point twice outside the plan"
    return Plan(cv, digit, point, sign, nb)


def fill_digits(count, lo, span):
    """`count` digits lo, lo + 1, ... cycling with period `span` (odd: a bucket then never meets a base point twice)"""
    assert span % 2 == 1 and lo + span <= (1 << 15)
    return lo + np.arange(count, dtype=np.int64) % span


def pm_kinds(length):
    """the +-P plans of a bucket of `length` entries: one point in every entry, the halves that cancel (even lengths) or
    differ by one (odd lengths: a of P, a - 1 of -P), and a split with two or three more of -P than of P"""
    a = length // 2
    out = [("pm", length, 0), ("pm", a, length - a) if length % 2 == 0 else ("pm", a + 1, a), ("pm", a - 1, length - a + 1)]
    return [(length, k) for k in out]


# ---- crafted GLV halves ----
def halves_to_scalar(cv, k1, k2):
    """k1 + k2 lambda mod r -- handed out only if `glv_decompose` returns exactly (k1, k2)"""
    k = (k1 + k2 * cv.lam) % cv.O.R
    assert cv.glv_decompose(k) == (k1, k2), (cv.name, hex(k1), hex(k2))
    return k


CRAFT_BITS = 121  # the magnitudes stay below 2^121: far inside the lattice's rounding region


def crafted_magnitudes(c):
    """magnitudes whose windows sit on the recoder's carry edge (window size c): every window B, every window B + 1, all
    ones, and chains of B-windows over a window below them that is 0, 1 (no carry) or B + 1 (carry), or over nothing"""
    nwin, B, full = CRAFT_BITS // c, 1 << (c - 1), (1 << c) - 1
    put = lambda ws: sum(v << (c * w) for w, v in ws)  # noqa: E731
    out = [put((w, B) for w in range(nwin)), put((w, B + 1) for w in range(nwin)), (1 << (nwin * c)) - 1]
    for ln in (1, 2, nwin - 2):
        for end in (0, 1, B + 1):
            # window 0 = the end, the chain above it, and a digit above the chain that takes the carry (or not)
            out.append(put([(0, end)] + [(w, B) for w in range(1, 1 + ln)] + [(1 + ln, full if ln == 2 else 5)]))
        out.append(put([(w, B) for w in range(ln)] + [(ln, B - 1)]))  # the chain starts at window 0
    return out


def crafted_scalars(cv, c):
    """every crafted magnitude on k1, on k2 and on both, under all four sign combinations -> [(scalar, k1, k2)]"""
    mags, out = crafted_magnitudes(c), []
    for i, m in enumerate(mags):
        m2 = mags[(i + 1) % len(mags)]
        for k1, k2 in ((m, 0), (-m, 0), (0, m), (0, -m), (m, m2), (m, -m2), (-m, m2), (-m, -m2)):
            out.append((halves_to_scalar(cv, k1, k2), k1, k2))
    return out


def scalar_entries(cv, k, c):
    """what `for_each_digit` emits for scalar k at window size c: [(half, window, |digit|, negative)]"""
    out = []
    for h, v in enumerate(cv.glv_decompose(k)):
        out += [(h, w, d, neg ^ (1 if v < 0 else 0)) for w, d, neg in for_each_digit(abs(v), c)]
    return out
