"""Shared by tests/test_multiopen_shapes.py (CPU) and tests/test_gpu_ipa_multiopen_shapes.py (GPU): a case builder for the
Bgh19 multi-open prover (csrc/ipa_multiopen.hip) and a catalogue of the query shapes at which the prover takes another path.
`ShapeCase` builds key, polynomials, blinds, x and the query list from a seeded `random.Random`; its oracle half runs
oracle/ipa.py, its device half takes a context.  Importing this module imports no torch and opens no device."""
import contextlib
import os
import random
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import ipa as I  # noqa: E402
import kzg as K  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402
import ntt_util  # noqa: E402
from snark_verifier_amd import poly as _poly  # noqa: E402
from test_gpu_ipa_create import BN, _dk, _gb, _points  # noqa: E402

CURVES = {"bn254": BN, "pallas": PA}
_MODS = {"bn254": O, "pallas": PA}
TERMS = _poly.LINCOMB_TERMS  # terms per pass of poly_enqueue_lincomb (csrc/poly.hpp: kPolyLincombTerms)
assert TERMS == 32  # the catalogue below is laid out around this value
MAX_K = 4  # the Python oracle and the verifier's commitments keep every shape of this file within a few seconds


@contextlib.contextmanager
def on_curve(curve):
    """the oracle's IPA module and the query-set grouping on `curve` inside the block, back on BN254 (their default) after"""
    I.use_curve(_MODS[curve])
    K.use_curve(_MODS[curve])
    try:
        yield
    finally:
        I.use_curve(O)
        K.use_curve(O)


def fe(v):
    return int(v).to_bytes(32, "little")


def horner(coeffs, z, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % r
    return acc


def shift(curve, j):
    """the j'th of a fixed list of distinct shifts: 1, then full-size field elements"""
    r = CURVES[curve].R
    return 1 if j == 0 else random.Random(repr(("multiopen-shift", curve, j))).randrange(2, r)


_KEYS = {}


def proof_len(k, n_sets):
    return 64 * k + 32 * n_sets + 160


class ShapeCase:
    """A zero-knowledge key of 2^k + 2 points, `n_polys` polynomials with blinds, x, the queries
    [(poly, shift, polys[poly](x * shift))] of `pairs`, and f_blind, p_bar, omega_bar: what the prover's rng would play.

    Overrides: `x`, `f_blind` (0 included), `zero_polys` (all-zero polynomials, the blinds stay), `replace` {query index:
    evaluation} and `extra` [(poly, shift, evaluation)] appended to the list, a duplicate for instance."""

    def __init__(self, curve, k, n_polys, pairs, tag, x=None, f_blind=None, zero_polys=False, replace=None, extra=()):
        assert 1 <= k <= MAX_K
        self.curve, self.k, self.n, self.n_polys, self.tag = curve, k, 1 << k, n_polys, tag
        cv = CURVES[curve]
        r, n = cv.R, self.n
        self.r = r
        rnd = random.Random(repr(("multiopen-shape", curve, k, tag)))
        if (curve, k) not in _KEYS:  # per curve and k: one key for every shape
            _KEYS[(curve, k)] = _points(curve, 900 + k, n + 2)
        pts = _KEYS[(curve, k)]
        self.key_bytes = _gb(curve, pts)
        with on_curve(curve):
            self.pk = I.IpaProvingKey(k, pts[:n], pts[n], pts[n + 1])
        self.polys = [[0 if zero_polys else rnd.randrange(r) for _ in range(n)] for _ in range(n_polys)]
        self.blinds = [rnd.randrange(1, r) for _ in range(n_polys)]
        drawn_x = rnd.randrange(1, r)
        self.x = drawn_x if x is None else x
        self.queries = [(p, s, self.eval_at(p, s)) for p, s in pairs]
        for at, ev in (replace or {}).items():
            self.queries[at] = (self.queries[at][0], self.queries[at][1], ev % r)
        self.queries += list(extra)
        drawn_f = rnd.randrange(1, r)
        self.f_blind = drawn_f if f_blind is None else f_blind
        self.omega_bar = rnd.randrange(r)
        self.p_bar = [rnd.randrange(r) for _ in range(n)]
        with on_curve(curve):
            self.sets = K.bdfg21_query_sets(self.queries)
        self.n_sets = len(self.sets)
        self._oracle, self._coms, self._dks = {}, None, {}

    def eval_at(self, poly, shift_):
        return horner(self.polys[poly], self.x * shift_ % self.r, self.r)

    def with_eval(self, changes):
        """the query list with {query index: evaluation} put in"""
        out = list(self.queries)
        for at, ev in changes.items():
            out[at] = (out[at][0], out[at][1], ev % self.r)
        return out

    # ---- the oracle half ------------------------------------------------------------------------------------------------
    def oracle(self, absorbed=b""):
        """the proof bytes of oracle.ipa.bgh19_create_proof; its rng replays f_blind, p_bar and omega_bar.  Computed once."""
        if absorbed not in self._oracle:
            with on_curve(self.curve):
                t = T.Blake2bTranscript(CURVES[self.curve])
                t.state.update(absorbed)
                play = iter([self.f_blind] + self.p_bar + [self.omega_bar])
                I.bgh19_create_proof(self.pk, self.polys, self.blinds, self.x, self.queries, t, lambda: next(play))
                self._oracle[absorbed] = t.finalize()
        return self._oracle[absorbed]

    def commitments(self):
        """pk.commit(polys[j], blinds[j]) of every polynomial: the oracle's own, unless a context has supplied them"""
        if self._coms is None:
            with on_curve(self.curve):
                self._coms = [self.pk.commit(p, b) for p, b in zip(self.polys, self.blinds)]
        return self._coms

    def verify(self, proof, absorbed=b""):
        """the oracle's verifier over the proof bytes -> the accumulator (xi, U); raises when the succinct check fails"""
        coms = self.commitments()
        with on_curve(self.curve):
            t = T.Blake2bTranscript(CURVES[self.curve], proof)
            t.state.update(absorbed)
            read = I.bgh19_read_proof(self.k, self.queries, t)
            acc = I.bgh19_verify(self.pk.g[0], self.pk.h, self.pk.s, [K.Msm.base(c) for c in coms], self.x, self.queries, read)
        return list(acc[0]), acc[1]

    def decides_on_host(self, acc):
        with on_curve(self.curve):
            return I.ipa_decide(self.pk.g, acc)

    # ---- the device half --------------------------------------------------------------------------------------------------
    def dk(self, ctx):
        """the deciding key of this case on `ctx`, made once per context"""
        if id(ctx) not in self._dks:
            self._dks[id(ctx)] = _dk(ctx, self.curve, self.key_bytes[:64 * self.n])
        return self._dks[id(ctx)]

    def commit_on(self, ctx):
        """the commitments from the device's batched commit, the blinds added on the host (as the existing `Case` does)"""
        if self._coms is None:
            mod = _MODS[self.curve]
            raw = ctx.ipa_commit_batch(self.dk(ctx), self.polys_bytes(), self.n)
            with on_curve(self.curve):
                self._coms = [mod.g1_add(mod.g1_from_bytes(raw[64 * j:64 * j + 64]), I._mul(self.pk.s, self.blinds[j]))
                              for j in range(self.n_polys)]
        return self._coms

    def polys_bytes(self):
        return b"".join(fe(c) for p in self.polys for c in p)

    def p_bar_bytes(self):
        return b"".join(fe(c) for c in self.p_bar)

    def device(self, MO, ctx, absorbed=b"", queries=None):
        """the host form -> (proof bytes, (xi, U))"""
        return MO.create_proof(ctx, self.dk(ctx), self.pk.h, self.pk.s, self.polys, self.blinds, self.x,
                               self.queries if queries is None else queries, self.f_blind, self.p_bar, self.omega_bar, absorbed)

    def device_dev(self, MO, ctx, d_polys, d_p_bar, absorbed=b""):
        """the device-resident form over the addresses of the polynomials (poly-major) and of p_bar"""
        return MO.create_proof_dev(ctx, self.dk(ctx), self.pk.h, self.pk.s, d_polys, self.n_polys, self.blinds, self.x, self.queries,
                                   self.f_blind, d_p_bar, self.omega_bar, absorbed)

    def decides(self, ctx, acc):
        cv = CURVES[self.curve]
        return ctx.ipa_decide_batch(self.dk(ctx), b"".join(cv.fe_to_bytes(v) for v in acc[0]), cv.g1_to_bytes(acc[1])) == [True]

    def close(self, ctx=None):
        """closes the deciding key on `ctx`, or on every context"""
        for key in [k for k in self._dks if ctx is None or k == id(ctx)]:
            self._dks.pop(key).close()


# ---- the catalogue ----------------------------------------------------------------------------------------------------------
# pairs: curve -> [(poly, shift)]; n_sets, largest_set and most_points are what the entry claims of its grouping
# (tests/test_multiopen_shapes.py holds the oracle and csrc/ipa_multiopen_sets.h to it); kw: the overrides of ShapeCase
Shape = namedtuple("Shape", "k n_polys pairs n_sets largest_set most_points reaches kw")


def _all_at_one(count):
    return lambda curve: [(p, 1) for p in range(count)]


def _own_shift(count):
    return lambda curve: [(p, shift(curve, p)) for p in range(count)]


def _two_big_sets(curve):
    """polynomials 0..39 at shift 1, ascending; 74 down to 40 at {1, w}, the odd ones asked as (w, 1): set 1 keeps the order
    (1, w) of polynomial 74, and polynomial 73 -- term 33 of its combination -- has its evaluations re-ordered.  The second
    set has polynomials of its own, 75 in all: a polynomial belongs to the one set of its shifts, so asking 35 of the first
    40 again at w would move them and leave no set with a second pass but theirs."""
    w = shift(curve, 1)
    out = [(p, 1) for p in range(40)]
    for p in range(74, 39, -1):
        out += [(p, w), (p, 1)] if p & 1 else [(p, 1), (p, w)]
    return out


def _regrouped(curve):
    """40 polynomials at shift 1, then 34 down to 0 again at w: those 35 leave for the set {1, w}, which polynomial 0 makes
    the first, and the evaluations at w sit at query indices 40 and up, in the other order"""
    w = shift(curve, 1)
    return [(p, 1) for p in range(40)] + [(p, w) for p in range(34, -1, -1)]


def _m_eq_n(k):
    n = 1 << k
    return lambda curve: ([(0, shift(curve, j)) for j in range(n)] + [(1, shift(curve, j)) for j in range(1, n)] + [(2, 1)])


def _rotations(curve):
    w = ntt_util.omega(curve, 4)
    r = CURVES[curve].R
    rot = {0: 1, 1: w, -1: pow(w, -1, r), 2: w * w % r}
    out = [(p, rot[0]) for p in range(12)]
    for p in (12, 13, 14):
        out += [(p, rot[0]), (p, rot[1])]
    for p in (15, 16):
        out += [(p, rot[0]), (p, rot[-1])]
    return out + [(17, rot[j]) for j in (0, 1, -1, 2)]


def _descending(curve):
    w, w2 = shift(curve, 1), shift(curve, 2)
    return [(7, 1), (7, w), (6, 1), (4, w), (4, 1), (2, 1), (1, 1), (1, w), (1, w2), (0, 1)]


def _dup(curve):
    w = shift(curve, 1)
    return [(0, 1), (1, 1), (1, w), (2, 1), (1, w)]  # query 4 repeats query 2; the entry replaces its evaluation


def _three_sets(curve):
    w, w2 = shift(curve, 1), shift(curve, 2)
    return [(0, 1), (1, 1), (1, w), (2, 1), (2, w), (2, w2)]


DUP_FIRST, DUP_SECOND = 2, 4  # the repeated (polynomial, shift) of `dup_first_wins`, as query indices

SHAPES = {
    "np32": Shape(3, 32, _all_at_one(32), 1, 32, 1,
                  "poly.hip poly_enqueue_lincomb: c = min(kPolyLincombTerms, count - j0), exactly one full pass for q", {}),
    "np33": Shape(3, 33, _all_at_one(33), 1, 33, 1,
                  "poly.hip poly_enqueue_lincomb: the second pass (j0 = 32, accumulate = 1) with one term; "
                  "ipa_multiopen.hip pl.idx / pl.scalars / pl.blind / vals[t] at index 32", {}),
    "np65": Shape(3, 65, _all_at_one(65), 1, 65, 1,
                  "poly.hip poly_enqueue_lincomb: a third pass (j0 = 64), PS_LC_IDX / PS_LC_SC staged three times", {}),
    "np40_two_sets": Shape(3, 75, _two_big_sets, 2, 40, 2,
                           "ipa_multiopen.hip the per-set loop: two sets whose second passes differ (8 and 3 terms), "
                           "st.evals[which][t] re-ordered at term 33 of set 1", {}),
    "np40_regrouped": Shape(3, 40, _regrouped, 2, 35, 2,
                            "ipa_multiopen_sets.h a later query moves a polynomial to another set; ipa_multiopen.hip "
                            "vals[t] from st.evals[which][1] past query 40 for a first set of 35 polynomials", {}),
    "S31": Shape(3, 31, _own_shift(31), 31, 1, 1,
                 "ipa_multiopen.hip f = sum x_2^j f_(S-1-j) with 31 terms, p = x_4^S f + ... with 32: one full pass", {}),
    "S32": Shape(3, 32, _own_shift(32), 32, 1, 1,
                 "ipa_multiopen.hip f's combination with 32 terms, p's with 33: p takes a second pass of one term", {}),
    "S33": Shape(3, 33, _own_shift(33), 33, 1, 1,
                 "ipa_multiopen.hip f's combination with 33 terms, p's with 34: both take a second pass", {}),
    "m5": Shape(3, 2, lambda curve: [(0, shift(curve, j)) for j in range(5)] + [(1, 1)], 2, 1, 5,
                "ipa_multiopen.hip the division chain: five divisions, dst ping-pongs d_t + 32 n / d_t twice each, then d_f; "
                "hipMemsetAsync(dst + 32 * len, ...) of the quotient tail at len = 7 .. 3", {}),
    "m_eq_n_k1": Shape(1, 3, _m_eq_n(1), 3, 1, 2,
                       "ipa_multiopen.hip `st.shifts.size() > n` at m = n = 2: the last division has len = 1, f_i = 0", {}),
    "m_eq_n_k2": Shape(2, 3, _m_eq_n(2), 3, 1, 4,
                       "ipa_multiopen.hip `st.shifts.size() > n` at m = n = 4; next to it a set of n - 1 points, len = 2 at last", {}),
    "m_eq_n_k3": Shape(3, 3, _m_eq_n(3), 3, 1, 8,
                       "ipa_multiopen.hip `st.shifts.size() > n` at m = n = 8: eight chained divisions down to the empty quotient", {}),
    "rotations": Shape(4, 18, _rotations, 4, 12, 4,
                       "ipa_multiopen.hip as a circuit asks: 12 columns at x, 3 at (x, w x), 2 at (x, x / w), one at four "
                       "rotations; n = 16", {}),
    "first_set_by_last_poly": Shape(3, 8, _descending, 3, 3, 3,
                                    "ipa_multiopen_sets.h per_poly in first-seen order: set 0 belongs to polynomial 7, "
                                    "polynomial 4 joins it re-ordered, 3 and 5 are in the array and never queried", {}),
    "dup_first_wins": Shape(3, 3, _dup, 2, 2, 2,
                            "ipa_multiopen_sets.h `if (!seen) ent->queries.push_back(q)`: the repeat's evaluation is wrong and unused",
                            {"replace_delta": {DUP_SECOND: 1}}),
    "x_zero": Shape(3, 3, lambda curve: [(0, 1), (1, shift(curve, 1)), (2, 1)], 2, 2, 1,
                    "ipa_multiopen.hip pts[t] = x * shift with x = 0: every point is 0, every division is by X", {"x": 0}),
    "zero_polys": Shape(3, 3, _three_sets, 3, 1, 3,
                        "ipa_multiopen.hip q = 0 and f = 0: ipa_enqueue_commit of the zero polynomial, f's commitment is "
                        "f_blind * S", {"zero_polys": True}),
}
DEV_FORM = ["np33", "S33", "m5", "m_eq_n_k2", "rotations"]  # the shapes the device-resident form is run at
assert all(s.k <= MAX_K for s in SHAPES.values())

_BUILT = {}


def build(curve, name, **kw):
    """the catalogue entry as a ShapeCase.  Without overrides the case is built once and shared: leave it unchanged."""
    sh = SHAPES[name]
    args = dict(sh.kw)
    args.update(kw)
    n_polys, pairs = args.pop("n_polys", sh.n_polys), args.pop("pairs", None)
    delta = args.pop("replace_delta", None)
    tag = args.pop("tag", name)

    def make():
        prs = sh.pairs(curve) if pairs is None else pairs
        c = ShapeCase(curve, sh.k, n_polys, prs, tag, **args)
        if delta:  # an evaluation moved off the polynomial's
            c.queries = c.with_eval({at: c.queries[at][2] + d for at, d in delta.items()})
        return c

    if kw:
        return make()
    if (curve, name) not in _BUILT:
        _BUILT[(curve, name)] = make()
    return _BUILT[(curve, name)]


def close_all(ctx=None):
    for c in _BUILT.values():
        c.close(ctx)


def largest(sets):
    """(set count, polynomials of the largest set, points of the set with the most) of a grouping"""
    return len(sets), max(len(st["polys"]) for st in sets), max(len(st["shifts"]) for st in sets)


# ---- the seeded differential ------------------------------------------------------------------------------------------------
RANDOM_LISTS = 12  # per curve and k


def random_pair_lists(curve, k):
    """RANDOM_LISTS lists of (poly, shift) pairs: 1 to 9 polynomials, 1 to 14 queries, shifts from a pool of five, repeats
    allowed.  A draw that asks one polynomial at more distinct shifts than it has coefficients is drawn again."""
    rnd = random.Random(repr(("multiopen-differential", curve, k)))
    pool = [shift(curve, j) for j in range(5)]
    out = []
    while len(out) < RANDOM_LISTS:
        n_polys = rnd.randrange(1, 10)
        pairs = [(rnd.randrange(n_polys), rnd.choice(pool)) for _ in range(rnd.randrange(1, 15))]
        if max(len({s for p, s in pairs if p == q}) for q in range(n_polys)) > (1 << k):
            continue
        out.append((n_polys, pairs))
    return out
