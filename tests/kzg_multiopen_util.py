"""A Python prover of the two KZG multi-open schemes, used as the expectation of the device provers
(include/snarkv_kzg_multiopen.h).  Under a toy secret s a commitment is [p(s)] G, so every output point follows from Horner
values at s, Lagrange values of the r_i at s and z', and one scalar multiplication: no polynomial is ever divided here, which
keeps the expectation independent of the device's route.  tests/test_kzg_multiopen_model.py pins these outputs with the
verifiers of oracle/kzg.py.

Also the host-side plan of csrc/kzg_multiopen_plan.h in Python integers, number for number: sets, polynomial order, the
scalars of the linear combinations, the coefficients of r, and after z' the scalars of L, its constant and Z_1(z').

Also `SHAPES`, the catalogue of query shapes at which the provers take another path (tests/test_kzg_multiopen_shapes.py on
the CPU, tests/test_gpu_kzg_multiopen_shapes.py on the device), the seeded query lists of the differential, and `Resident` /
`check_case`, the device flow the GPU tests share.  Importing this module imports no torch and opens no device.
TEST INFRASTRUCTURE ONLY."""
import os
import random
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import kzg as K  # noqa: E402

R = O.R
GWC19, BDFG21 = 0, 1
_GEN = O.g1_to_bytes(O.G1_GEN)


def inv(a):
    return pow(a % R, -1, R)


def horner(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def mulg(k):
    """[k] G as 64 bytes; the identity is 64 zero bytes"""
    k %= R
    return b"\x00" * 64 if k == 0 else C.g1_mul(_GEN, O.fe_to_bytes(k))


def srs(s, n):
    """[s^i] G, i < n, packed"""
    out, p = [], 1
    for _ in range(n):
        out.append(mulg(p))
        p = p * s % R
    return b"".join(out)


def lagrange_value(points, values, x):
    """the polynomial of degree < m through (points[t], values[t]), at x"""
    acc = 0
    for j, (pj, vj) in enumerate(zip(points, values)):
        num = den = 1
        for i, pi in enumerate(points):
            if i != j:
                num, den = num * (x - pi) % R, den * (pj - pi) % R
        acc = (acc + vj * num * inv(den)) % R
    return acc


def interpolate(points, values):
    """its coefficients, lowest first"""
    m = len(points)
    out = [0] * m
    for j in range(m):
        num, den = [1], 1
        for i in range(m):
            if i != j:
                nxt = [0] * (len(num) + 1)
                for t, c in enumerate(num):
                    nxt[t + 1] = (nxt[t + 1] + c) % R
                    nxt[t] = (nxt[t] - points[i] * c) % R
                num, den = nxt, den * (points[j] - points[i]) % R
        f = values[j] * inv(den) % R
        for t in range(m):
            out[t] = (out[t] + num[t] * f) % R
    return out


def sets_of(mos, queries):
    """the query sets in one shape for both schemes: {"shifts": [..], "polys": [..], "evals": [[per shift] per polynomial]}"""
    if mos == GWC19:
        return [{"shifts": [st["shift"]], "polys": st["polys"], "evals": [[e] for e in st["evals"]]} for st in K.gwc19_query_sets(queries)]
    return K.bdfg21_query_sets(queries)


def plan(mos, queries, z, c):
    """per set: polys, scalars c^j, points z shift_t, r (the coefficients of the interpolation of the c-combined evaluations)"""
    out = []
    for st in sets_of(mos, queries):
        pc = K.powers(c, len(st["polys"]))
        points = [z * sh % R for sh in st["shifts"]]
        vals = [sum(pc[j] * st["evals"][j][t] for j in range(len(pc))) % R for t in range(len(points))]
        out.append({"polys": list(st["polys"]), "scalars": pc, "points": points, "vals": vals, "r": interpolate(points, vals)})
    return out


def plan_finish(pl, gamma, z_prime):
    """Bdfg21 after z': L = sum scalars[j] polys[idx[j]] - z1 h - constant"""
    idx, scalars, constant, z1 = [], [], 0, None
    for i, st in enumerate(pl):
        zi = 1
        for p in st["points"]:
            zi = zi * (z_prime - p) % R
        if z1 is None:
            z1 = zi
        f = pow(gamma, i, R) * z1 * inv(zi) % R
        constant = (constant + f * horner(st["r"], z_prime)) % R
        idx += st["polys"]
        scalars += [f * sc % R for sc in st["scalars"]]
    return {"idx": idx, "scalars": scalars, "constant": constant, "z1": z1}


def gwc19_prove(s, polys, z, queries, v):
    """[W_k]: W_k = [(sum_i v^i p_i(s) - sum_i v^i e_i) / (s - z shift_k)] G"""
    ws = []
    for st in K.gwc19_query_sets(queries):
        pv = K.powers(v, len(st["polys"]))
        num = sum(pvi * (horner(polys[p], s) - e) for p, e, pvi in zip(st["polys"], st["evals"], pv)) % R
        ws.append(mulg(num * inv(s - z * st["shift"])))
    return ws


def bdfg21_h_at(s, polys, z, queries, mu, gamma):
    """h(s) = sum_i gamma^i (q_i(s) - r_i(s)) / Z_i(s), and per set (q_i(s), points, mu-combined evaluations)"""
    h, per_set = 0, []
    for i, st in enumerate(K.bdfg21_query_sets(queries)):
        pm = K.powers(mu, len(st["polys"]))
        points = [z * sh % R for sh in st["shifts"]]
        vals = [sum(pm[j] * st["evals"][j][t] for j in range(len(pm))) % R for t in range(len(points))]
        q_s = sum(pmj * horner(polys[p], s) for p, pmj in zip(st["polys"], pm)) % R
        z_s = 1
        for p in points:
            z_s = z_s * (s - p) % R
        h = (h + pow(gamma, i, R) * (q_s - lagrange_value(points, vals, s)) * inv(z_s)) % R
        per_set.append((q_s, points, vals))
    return h, per_set


def bdfg21_prove(s, polys, z, queries, mu, gamma, draw_z_prime):
    """(W, z', W'): W = [h(s)] G, z' = draw_z_prime(W), W' = [L(s) / (s - z')] G with
    L(s) = sum_i gamma^i (Z_1(z') / Z_i(z')) (q_i(s) - r_i(z')) - Z_1(z') h(s)"""
    h, per_set = bdfg21_h_at(s, polys, z, queries, mu, gamma)
    w = mulg(h)
    z_prime = draw_z_prime(w) % R
    big_l, z1 = 0, None
    for i, (q_s, points, vals) in enumerate(per_set):
        zi = 1
        for p in points:
            zi = zi * (z_prime - p) % R
        if z1 is None:
            z1 = zi
        big_l = (big_l + pow(gamma, i, R) * z1 * inv(zi) * (q_s - lagrange_value(points, vals, z_prime))) % R
    big_l = (big_l - z1 * h) % R
    return w, z_prime, mulg(big_l * inv(s - z_prime))


def commitments(s, polys):
    """[p(s)] G per polynomial, as points (None: the identity)"""
    return [O.g1_from_bytes(mulg(horner(p, s))) for p in polys]


def with_evals(polys, z, pairs):
    """[(poly, shift)] -> [(poly, shift, polys[poly](z shift))]"""
    return [(p, sh, horner(polys[p], z * sh % R)) for p, sh in pairs]


def standard_plonk_instance(rng, n, n_polys=17):
    """random polynomials of n coefficients in the query shape of oracle/kzg.py::standard_plonk_queries, with z"""
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_polys)]
    z = rng.randrange(1, R)
    return polys, z, with_evals(polys, z, K.standard_plonk_queries(rng, n_polys))


def draw_from(tag):
    """a deterministic stand-in for the transcript: z' from the bytes of W"""
    import hashlib

    return lambda w: int.from_bytes(hashlib.sha256(tag.encode() + bytes(w)).digest(), "little") % R


def set_shape_cases(rng):
    """name -> (polys, z, queries): the set shapes at which the provers take another path"""
    def rand_polys(count, n):
        return [[rng.randrange(R) for _ in range(n)] for _ in range(count)]

    cases = {}
    w1, w2 = rng.randrange(2, R), rng.randrange(2, R)
    polys, z = rand_polys(1, 5), rng.randrange(1, R)
    cases["one polynomial, one query"] = (polys, z, with_evals(polys, z, [(0, 1)]))
    polys, z = rand_polys(40, 64), rng.randrange(1, R)  # 40 terms: two passes of the linear combination
    cases["40 polynomials in one set"] = (polys, z, with_evals(polys, z, [(p, w1) for p in range(40)]))
    polys, z = rand_polys(3, 9), rng.randrange(1, R)
    cases["a pair given twice"] = (polys, z, with_evals(polys, z, [(0, 1), (1, 1), (1, w1), (0, 1), (2, w1), (1, w1)]))
    polys, z = rand_polys(2, 3), rng.randrange(1, R)  # as many points as coefficients: q - r = 0, the zero quotient
    three = [(0, 1), (0, w1), (0, w2)]
    cases["three points at n = 3, and a second set"] = (polys, z, with_evals(polys, z, three + [(1, w1)]))
    cases["three points at n = 3, alone"] = (polys[:1], z, with_evals(polys, z, three))
    polys, z = rand_polys(2, 1), rng.randrange(1, R)  # constants: every quotient is empty, every output the identity
    cases["constants, n = 1"] = (polys, z, with_evals(polys, z, [(0, 1), (1, w1)]))
    return cases


# ---- the plan's refusals, as the header states them ---------------------------------------------------------------------------
PLAN_OK, PLAN_BAD_MOS, PLAN_COINCIDE, PLAN_TOO_MANY_POINTS, PLAN_ZERO_Z = range(5)  # kzgplan::kOk .. kZeroZ


def plan_status(mos, queries, n, z, z_prime=None):
    """(status, set) of kzg_plan_build and, with z_prime, kzg_plan_finish: sets in order, per set first the count of its points,
    then their distinctness; after z', the first set one of whose points is z'"""
    sets = sets_of(mos, queries)
    for i, st in enumerate(sets):
        if len(st["shifts"]) > n:
            return PLAN_TOO_MANY_POINTS, i
        if len({z * sh % R for sh in st["shifts"]}) < len(st["shifts"]):
            return PLAN_COINCIDE, i
    if z_prime is not None:
        for i, st in enumerate(sets):
            if any((z_prime - z * sh) % R == 0 for sh in st["shifts"]):
                return PLAN_ZERO_Z, i
    return PLAN_OK, 0


def first_bad_set(mos, polys, z, queries, c):
    """the first set whose c-combined polynomial misses a c-combined evaluation at a point of the set -- the set whose
    division leaves a remainder, which the provers name -- or None.  (Under a known secret the Python prover above solves a W
    for any evaluations; this is the model of the refusal.)"""
    for i, st in enumerate(plan(mos, queries, z, c)):
        for point, val in zip(st["points"], st["vals"]):
            if sum(sc * horner(polys[p], point) for sc, p in zip(st["scalars"], st["polys"])) % R != val:
                return i
    return None


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
SECRET = 0x7A11_5EC2_E7
# The secret of the one shape whose SRS would otherwise take minutes (n = 65 537; a scalar multiplication of the C oracle takes
# about 4 ms): an element of order 983, s = 5^((r - 1) / 983).  983 divides r - 1, s != 1 and s^983 = 1, so [s^i] G has the
# period 983 and the SRS is 983 distinct points tiled to n.  983 is odd and prime: no power-of-two stride is a multiple of it,
# so a coefficient misplaced by a block, a wave or a scan segment of the device meets another power of s and p(s) changes.  The
# repeated base points send equal points into one bucket of the MSM; that is legal input (tests/test_gpu_robustness.py runs
# MSMs over repeated points at scale), so a mismatch at this shape is the prover's, and a fault there would be the MSM's.
ORDER_983 = 983
SECRET_983 = pow(5, (R - 1) // ORDER_983, R)
assert (R - 1) % ORDER_983 == 0 and SECRET_983 != 1 and pow(SECRET_983, ORDER_983, R) == 1
TERMS = 32     # terms per pass of poly_enqueue_lincomb (csrc/poly.hpp: kPolyLincombTerms; snark_verifier_amd.poly.LINCOMB_TERMS)
MAX_JOBS = 64  # jobs per round of launch_msm_pippenger_many (include/snarkv_amd.h: SNARKV_MANY_MAX_JOBS)

# what an entry claims of its grouping under one scheme; l_terms is the number of terms of Bdfg21's L (None under Gwc19)
Claim = namedtuple("Claim", "n_sets largest_set most_points l_terms")
# pairs: () -> [(poly, shift)]; kw: "z", "secret", "polys" (rng, n) -> the polynomials, "identity" the Gwc19 outputs that are
# the identity
Shape = namedtuple("Shape", "n n_polys pairs gwc19 bdfg21 reaches kw")

_SRS = {}


def srs_of(secret, n):
    """the SRS of `secret` with n points, the powers computed once per secret; under SECRET_983 one period, tiled"""
    if secret == SECRET_983:
        if secret not in _SRS:
            _SRS[secret] = srs(secret, ORDER_983)
        return (_SRS[secret] * (n // ORDER_983 + 1))[:64 * n]
    if len(_SRS.get(secret, b"")) < 64 * n:
        _SRS[secret] = srs(secret, max(n, 1000))
    return _SRS[secret][:64 * n]


def shift(j):
    """the j'th of a fixed list of distinct shifts: 1, then full-size field elements"""
    return 1 if j == 0 else random.Random(repr(("kzg-multiopen-shift", j))).randrange(2, R)


def omega16():
    """a 16th root of unity of BN254's Fr: the rotation of a domain of 16 rows"""
    import ntt_util

    return ntt_util.omega("bn254", 4)


def _all_at_one(count):
    return lambda: [(p, 1) for p in range(count)]


def _own_shift(count):
    return lambda: [(p, shift(p)) for p in range(count)]


def _two_sets(first, second):
    """`first` polynomials at {1}, then `second` at {1, w}"""
    def pairs():
        out = [(p, 1) for p in range(first)]
        for p in range(first, first + second):
            out += [(p, 1), (p, shift(1))]
        return out
    return pairs


def _points_on_one(m, others):
    """polynomial 0 at the first m shifts, then `others` [(poly, shift index)]"""
    return lambda: [(0, shift(j)) for j in range(m)] + [(p, shift(j)) for p, j in others]


def _rotations():
    """tests/multiopen_util.py::_rotations over BN254's Fr: 12 columns at x, 3 at (x, w x), 2 at (x, x / w), one at four"""
    w = omega16()
    rot = {0: 1, 1: w, -1: pow(w, -1, R), 2: w * w % R}
    out = [(p, rot[0]) for p in range(12)]
    for p in (12, 13, 14):
        out += [(p, rot[0]), (p, rot[1])]
    for p in (15, 16):
        out += [(p, rot[0]), (p, rot[-1])]
    return out + [(17, rot[j]) for j in (0, 1, -1, 2)]


def _zero_job_polys(rng, n):
    """0, 1: constants in n coefficients; 2: the zero polynomial; 3, 4: random"""
    return ([[rng.randrange(1, R)] + [0] * (n - 1) for _ in range(2)] + [[0] * n]
            + [[rng.randrange(R) for _ in range(n)] for _ in range(2)])


def _np(count, passes):
    return Shape(8, count, _all_at_one(count), Claim(1, count, 1, None), Claim(1, count, 1, count),
                 "poly.hip poly_enqueue_lincomb: %s of a set's combination (c = min(kPolyLincombTerms, count - j0)); "
                 "kzg_multiopen_plan.h pc[j] and vals[t] up to j = %d; L has the same terms" % (passes, count - 1), {})


SHAPES = {
    "np32": _np(32, "exactly one full pass"),
    "np33": _np(33, "a second pass (j0 = 32, accumulate) of one term"),
    "np65": _np(65, "a third pass (j0 = 64)"),
    "L32": Shape(8, 32, _two_sets(16, 16), Claim(2, 32, 1, None), Claim(2, 16, 2, 32),
                 "kzg_multiopen.hip bdfg21_create_proof: poly_enqueue_lincomb(pl.idx ...) for L with exactly 32 terms from two "
                 "sets of one pass each; Gwc19's set of shift 1 has all 32", {}),
    "L33": Shape(8, 33, _two_sets(16, 17), Claim(2, 33, 1, None), Claim(2, 17, 2, 33),
                 "kzg_multiopen.hip bdfg21_create_proof: L takes a second pass whose one term is the last polynomial of the "
                 "second set (kzg_plan_finish: f of set 1 times mu^16); Gwc19's set of shift 1 takes a second pass too", {}),
    "S64": Shape(8, 64, _own_shift(64), Claim(64, 1, 1, None), Claim(64, 1, 1, 64),
                 "msm_api.hip launch_msm_pippenger_many: G = min(count, SNARKV_MANY_MAX_JOBS) = 64 jobs in one round; "
                 "kzg_multiopen.hip h over 64 sets by k_kzg_axpy_sub, L of two full passes", {}),
    "S65": Shape(8, 65, _own_shift(65), Claim(65, 1, 1, None), Claim(65, 1, 1, 65),
                 "msm_api.hip launch_msm_pippenger_many: rounds = 2, G = 33: the second round of 32 jobs reuses the grids after "
                 "join_and_fork and writes d_out + 64 * 33; kzg_multiopen.hip h over 65 sets, L of 65 terms", {}),
    "m3_257": Shape(257, 2, _points_on_one(3, [(1, 1)]), Claim(3, 2, 1, None), Claim(2, 1, 3, 2),
                    "kzg_multiopen.hip KzgRun::divide: three divisions at len = 257, 256, 255 (poly.hip div_linear: two blocks of "
                    "the scan, exactly one, one short of one), the memset of the top 1, 2, 3 coefficients", {}),
    "m5_1000": Shape(1000, 2, _points_on_one(5, [(1, 0), (1, 1)]), Claim(5, 2, 1, None), Claim(2, 1, 5, 2),
                     "kzg_multiopen.hip KzgRun::divide: five divisions, `to` goes to each half of d_t twice and the last hop "
                     "leaves the lower half for dst (an even m, as the two points of the second set, leaves the upper one)", {}),
    "m3_65537": Shape(65537, 2, _points_on_one(3, [(1, 0), (1, 1)]), Claim(3, 2, 1, None), Claim(2, 1, 3, 2),
                      "poly.hip poly_enqueue_div_linear at len = 65 537, 65 536, 65 535: three scan levels, then two at 256^2 and "
                      "below; kzg_multiopen.hip L / (X - z') at 65 537", {"secret": SECRET_983}),
    "m_eq_n_2": Shape(2, 2, _points_on_one(2, [(1, 1)]), Claim(2, 2, 1, None), Claim(2, 1, 2, 2),
                      "kzg_multiopen.hip KzgRun::divide: m = n = 2, the last division has len = 1 and `to = nullptr`, the memset "
                      "clears all of dst: W's share of that set is zero; kzg_multiopen_plan.h `m > n` does not fire", {}),
    "m_eq_n_17": Shape(17, 2, _points_on_one(17, [(1, 1)]), Claim(17, 2, 1, None), Claim(2, 1, 17, 2),
                       "kzg_multiopen.hip KzgRun::divide: seventeen chained divisions down to the empty quotient; fr_host.h "
                       "h_interpolate over 17 points", {}),
    "zero_job": Shape(64, 5, lambda: [(0, shift(1)), (1, shift(1)), (2, shift(1)), (3, shift(2)), (4, shift(2))],
                      Claim(2, 3, 1, None), Claim(2, 3, 1, 5),
                      "kzg_multiopen.hip gwc19_create_proof: job 0 of the batch has only zero scalars (constants minus their "
                      "evaluations, and a zero polynomial) next to a live job: W_0 is the identity, W_1 is not",
                      {"polys": _zero_job_polys, "identity": (0,)}),
    "z_zero": Shape(8, 3, _own_shift(3), Claim(3, 1, 1, None), Claim(3, 1, 1, 3),
                    "kzg_multiopen_plan.h pts[t] = z * shift with z = 0: every point is 0, in different sets, every division is "
                    "by X; h_interpolate sees one point per set, so nothing coincides", {"z": 0}),
    "rotations": Shape(300, 18, _rotations, Claim(4, 18, 1, None), Claim(4, 12, 4, 18),
                       "kzg_multiopen.hip as a circuit asks: 12 columns at z, 3 at (z, w z), 2 at (z, z / w), one at four "
                       "rotations; Gwc19's sets have 18, 4, 3 and 1 polynomials", {}),
}


class Case:
    """a catalogue entry with its numbers: polynomials, z, the queries with Horner's evaluations, the secret of its SRS"""

    def __init__(self, name, sh):
        rng = random.Random(repr(("kzg-multiopen-shape", name)))
        self.name, self.n, self.secret = name, sh.n, sh.kw.get("secret", SECRET)
        make = sh.kw.get("polys", lambda r, n: [[r.randrange(R) for _ in range(n)] for _ in range(sh.n_polys)])
        self.polys = make(rng, sh.n)
        drawn = rng.randrange(1, R)
        self.z = sh.kw.get("z", drawn)
        self.pairs = sh.pairs()
        self.queries = with_evals(self.polys, self.z, self.pairs)
        self.identity = tuple(sh.kw.get("identity", ()))
        assert len(self.polys) == sh.n_polys and all(len(p) == sh.n for p in self.polys)


_BUILT = {}


def build(name):
    """the catalogue entry as a Case, built once and shared: leave it unchanged"""
    if name not in _BUILT:
        _BUILT[name] = Case(name, SHAPES[name])
    return _BUILT[name]


def claim_of(mos, queries):
    """what a query list's grouping is under `mos`, in the shape of `Claim`"""
    sets = sets_of(mos, queries)
    return Claim(len(sets), max(len(st["polys"]) for st in sets), max(len(st["shifts"]) for st in sets),
                 None if mos == GWC19 else sum(len(st["polys"]) for st in sets))


# ---- the seeded differential --------------------------------------------------------------------------------------------------
RANDOM_LISTS = 12  # per n
RANDOM_NS = (5, 300)
# The seed is chosen on the CPU, by the model alone (tests/test_kzg_multiopen_shapes.py asserts it): at most a quarter of the
# lists of an n may be ones the plan refuses, and at n = 5 some list asks one polynomial at all five shifts of the pool.  With
# five shifts a set has at most five points, so at these n the plan refuses none: m = n = 5 is the edge they reach.
RANDOM_SEED = 0


def random_query_lists(n):
    """RANDOM_LISTS cases (polys, z, queries): 1 to 9 polynomials of n coefficients, 1 to 14 queries, shifts from a pool of
    five, repeats allowed.  Nothing is drawn again: a list the plan refuses stays, and the device must refuse it alike."""
    rnd = random.Random(repr(("kzg-multiopen-differential", RANDOM_SEED, n)))
    pool = [shift(j) for j in range(5)]
    out = []
    for _ in range(RANDOM_LISTS):
        n_polys = rnd.randrange(1, 10)
        pairs = [(rnd.randrange(n_polys), rnd.choice(pool)) for _ in range(rnd.randrange(1, 15))]
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(n_polys)]
        z = rnd.randrange(1, R)
        out.append((polys, z, with_evals(polys, z, pairs)))
    return out


# ---- the device flow the GPU tests share --------------------------------------------------------------------------------------
GUARD = 4096  # bytes of 0xA5 on both sides of a guarded device input; a multiple of the 16-byte alignment the _dev forms ask


def pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def to_dev(raw):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


class Resident:
    """polynomials and SRS on the device, and the queries with the evaluations the device computed
    (`poly_batch.eval_many_dev`).  With `guard` the two inputs lie between GUARD bytes of 0xA5 each side; `unchanged()` reads
    them back whole."""

    def __init__(self, ctx, srs_bytes, polys, z, pairs, guard=False):
        import torch

        from snark_verifier_amd import poly_batch

        self.polys, self.z, self.n = polys, z, len(polys[0])
        self.srs = srs_bytes[:64 * self.n]
        assert len(self.srs) == 64 * self.n
        pad = b"\xa5" * (GUARD if guard else 0)
        self._host = [pad + self.srs + pad, pad + b"".join(pack(p) for p in polys) + pad]
        self._bufs = [to_dev(raw) for raw in self._host]
        self.d_srs, self.d_polys = (buf[len(pad):len(buf) - len(pad)] for buf in self._bufs)
        assert self.d_srs.data_ptr() % 16 == 0 and self.d_polys.data_ptr() % 16 == 0
        shifts = sorted({sh for _, sh in pairs})
        d_points = to_dev(pack([z * sh % R for sh in shifts]))
        d_out = torch.zeros(32 * len(pairs), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        poly_batch.eval_many_dev(ctx, self.d_polys, self.n, len(polys), d_points, len(shifts), [p for p, _ in pairs],
                                 [shifts.index(sh) for _, sh in pairs], d_out)
        ctx.sync()
        raw = d_out.cpu().numpy().tobytes()
        self.queries = [(p, sh, int.from_bytes(raw[32 * i:32 * i + 32], "little")) for i, (p, sh) in enumerate(pairs)]

    def unchanged(self):
        import torch

        torch.cuda.synchronize()
        return all(buf.cpu().numpy().tobytes() == raw for buf, raw in zip(self._bufs, self._host))


def challenges(tag):
    """(v, u, mu, gamma) of a tag: the caller's transcript, seeded"""
    rng = random.Random("challenges " + tag)
    return tuple(rng.randrange(1, R) for _ in range(4))


def check_case(ctx, KM, dk, secret, res, tag, forms=("host", "dev"), decide=True):
    """both schemes in the given forms on `res` against the Python prover under `secret`, byte for byte; with `decide` the
    oracle's verifiers give lhs == [s] rhs on the outputs and the device's decide accepts lhs || rhs and rejects lhs + G.
    `decide` may name the schemes to decide: ("gwc19", "bdfg21").  -> (ws, (w, z', w'))"""
    polys, z, queries = res.polys, res.z, res.queries
    assert queries == with_evals(polys, z, [(p, sh) for p, sh, _ in queries])  # the device's evaluations are Horner's
    v, u, mu, gamma = challenges(tag)
    draw = draw_from(tag)
    want_ws = gwc19_prove(secret, polys, z, queries, v)
    want_w, want_zp, want_wp = bdfg21_prove(secret, polys, z, queries, mu, gamma, draw)
    for form in forms:
        if form == "host":
            ws = KM.gwc19_create_proof(ctx, res.srs, polys, z, queries, v)
            w, zp, wp = KM.bdfg21_create_proof(ctx, res.srs, polys, z, queries, mu, gamma, draw)
        else:
            ws = KM.gwc19_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, len(polys), z, queries, v)
            w, zp, wp = KM.bdfg21_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, len(polys), z, queries, mu, gamma, draw)
        assert ws == want_ws, (tag, form)
        assert (w, zp, wp) == (want_w, want_zp, want_wp), (tag, form)
    assert len(ws) == KM.n_sets(KM.MOS_GWC19, queries)
    schemes = ("gwc19", "bdfg21") if decide is True else tuple(decide or ())
    if not schemes:
        return ws, (w, zp, wp)
    cms = [K.Msm.base(c) for c in commitments(secret, polys)]
    pt = O.g1_from_bytes
    pairs = []
    if "gwc19" in schemes:
        pairs.append(K.gwc19_verify(O.G1_GEN, cms, z, queries, v, [pt(x) for x in ws], u))
    if "bdfg21" in schemes:
        pairs.append(K.bdfg21_verify(O.G1_GEN, cms, z, queries, mu, gamma, pt(w), zp, pt(wp)))
    for lhs, rhs in pairs:
        assert rhs is not None and lhs == O.g1_mul(rhs, secret), tag
        assert ctx.decide(dk, O.g1_to_bytes(lhs) + O.g1_to_bytes(rhs)), tag
        assert not ctx.decide(dk, O.g1_to_bytes(O.g1_add(lhs, O.G1_GEN)) + O.g1_to_bytes(rhs)), tag
    return ws, (w, zp, wp)
