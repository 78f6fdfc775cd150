"""CPU: the catalogue of query shapes in tests/kzg_multiopen_util.py::SHAPES is what it says, before any kernel runs.

  * at every entry the Python prover satisfies the verifiers of oracle/kzg.py under the entry's secret: lhs == [s] rhs.  The
    expectations of tests/test_gpu_kzg_multiopen_shapes.py stay pinned by the oracle, never by the code under test.
  * the oracle's groupings (gwc19_query_sets / bdfg21_query_sets) have the set count, the largest set, the most points and
    the terms of L that the entry claims, and the counts sit where the catalogue is laid out around them (32 terms a pass, 64
    jobs a round).
  * the compiled plan (csrc/kzg_multiopen_plan.h through tests/hosttest/hosttest_kzg_open.cpp) equals the util's number for
    number at every entry, both schemes, L included.
  * the plan's refusals, with the set each names: coinciding points at z = 0 and for two encodings of one shift, m = n + 1,
    z' on the first and on the last point of the last set.
  * what the GPU tests rely on in named entries, in the repeated query with a wrong second evaluation, and in the seeded
    lists of the differential."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import kzg as K  # noqa: E402
import kzg_multiopen_util as U  # noqa: E402
from test_kzg_multiopen_model import host_plan  # noqa: E402

R = O.R
ZERO64 = b"\x00" * 64
NAMES = list(U.SHAPES)


def _pt(b):
    return O.g1_from_bytes(b)


def verifies(secret, polys, z, queries, seed):
    """the Python prover's outputs under both verifiers of the oracle -> (ws, (w, z', w'))"""
    rng = random.Random("verify " + seed)
    v, u, mu, gamma = (rng.randrange(1, R) for _ in range(4))
    cms = [K.Msm.base(c) for c in U.commitments(secret, polys)]
    ws = U.gwc19_prove(secret, polys, z, queries, v)
    lhs, rhs = K.gwc19_verify(O.G1_GEN, cms, z, queries, v, [_pt(w) for w in ws], u)
    ok_g = lhs == (O.g1_mul(rhs, secret) if rhs is not None else None)
    w, z_prime, w_prime = U.bdfg21_prove(secret, polys, z, queries, mu, gamma, U.draw_from(seed))
    lhs, rhs = K.bdfg21_verify(O.G1_GEN, cms, z, queries, mu, gamma, _pt(w), z_prime, _pt(w_prime))
    ok_b = lhs == (O.g1_mul(rhs, secret) if rhs is not None else None)
    return ok_g, ok_b, ws, (w, z_prime, w_prime)


def test_the_catalogue_is_laid_out_around_the_pass_length_and_the_round_size():
    from snark_verifier_amd import poly

    assert poly.LINCOMB_TERMS == U.TERMS == 32
    with open(os.path.join(ROOT, "include", "snarkv_amd.h")) as f:
        assert "#define SNARKV_MANY_MAX_JOBS %d\n" % U.MAX_JOBS in f.read()
    sh = U.SHAPES
    assert [sh[n].bdfg21.largest_set for n in ("np32", "np33", "np65")] == [U.TERMS, U.TERMS + 1, 2 * U.TERMS + 1]
    assert [sh[n].bdfg21.l_terms for n in ("L32", "L33")] == [U.TERMS, U.TERMS + 1]
    assert all(sh[n].bdfg21.largest_set <= U.TERMS for n in ("L32", "L33"))
    assert [sh[n].gwc19.n_sets for n in ("S64", "S65")] == [U.MAX_JOBS, U.MAX_JOBS + 1]
    assert [(sh[n].n, sh[n].bdfg21.most_points) for n in ("m3_257", "m3_65537")] == [(257, 3), (256 * 256 + 1, 3)]
    assert sh["m5_1000"].bdfg21.most_points == 5
    for n in (2, 17):
        assert sh["m_eq_n_%d" % n].n == sh["m_eq_n_%d" % n].bdfg21.most_points == n
    assert all(s.reaches and s.gwc19.most_points == 1 and s.gwc19.l_terms is None for s in sh.values())
    # the toy secret of the large shape: of order 983, an odd prime
    assert U.SECRET_983 != 1 and pow(U.SECRET_983, 983, R) == 1 and (R - 1) % 983 == 0
    assert all(983 % d for d in range(2, 32)) and [n for n in NAMES if sh[n].kw.get("secret")] == ["m3_65537"]


@pytest.mark.parametrize("name", NAMES)
def test_the_grouping_is_what_the_entry_claims(name):
    c, sh = U.build(name), U.SHAPES[name]
    assert U.claim_of(U.GWC19, c.queries) == sh.gwc19
    assert U.claim_of(U.BDFG21, c.queries) == sh.bdfg21
    assert sh.bdfg21.most_points <= c.n  # within the plan's `m > n`
    assert len({q[1] for q in c.queries}) == len({q[1] % R for q in c.queries})  # the shifts are distinct as values
    assert {q[0] for q in c.queries} == set(range(sh.n_polys))
    assert U.plan_status(U.GWC19, c.queries, c.n, c.z) == U.plan_status(U.BDFG21, c.queries, c.n, c.z) == (U.PLAN_OK, 0)


@pytest.mark.parametrize("name", NAMES)
def test_the_expected_points_satisfy_the_oracle_verifiers(name):
    c = U.build(name)
    ok_g, ok_b, ws, (w, _, w_prime) = verifies(c.secret, c.polys, c.z, c.queries, name)
    assert ok_g and ok_b
    # the identity is where the entry says, and nowhere else
    assert [i for i, x in enumerate(ws) if x == ZERO64] == list(c.identity)
    assert w != ZERO64 and w_prime != ZERO64
    # a wrong evaluation does not verify: the expectation is not vacuous
    bad = c.queries[:-1] + [(c.queries[-1][0], c.queries[-1][1], (c.queries[-1][2] + 1) % R)]
    cms = [K.Msm.base(x) for x in U.commitments(c.secret, c.polys)]
    lhs, rhs = K.gwc19_verify(O.G1_GEN, cms, c.z, bad, 3, [_pt(x) for x in U.gwc19_prove(c.secret, c.polys, c.z, c.queries, 3)], 5)
    assert lhs != (O.g1_mul(rhs, c.secret) if rhs is not None else None)


@pytest.mark.parametrize("name", NAMES)
def test_the_host_plan_equals_the_python_plan_number_for_number(name):
    c = U.build(name)
    rng = random.Random("plan " + name)
    v, mu, gamma, z_prime = (rng.randrange(1, R) for _ in range(4))
    for mos, ch in ((U.GWC19, v), (U.BDFG21, mu)):
        want = U.plan(mos, c.queries, c.z, ch)
        bd = mos == U.BDFG21
        status, _, sets, big_l = host_plan(mos, c.queries, c.n, c.z, ch, gamma if bd else None, z_prime if bd else None)
        assert status == 0
        assert sets == [{k: st[k] for k in ("polys", "scalars", "points", "r")} for st in want], (name, mos)
        if bd:
            want_l = U.plan_finish(want, gamma, z_prime)
            assert big_l == want_l, name
            assert len(want_l["idx"]) == U.SHAPES[name].bdfg21.l_terms
            # the first set's factor is 1: its terms of L carry the bare mu^j
            assert big_l["scalars"][:len(want[0]["scalars"])] == want[0]["scalars"]


def test_the_plan_refuses_with_the_right_set():
    w, w2 = U.shift(1), U.shift(2)
    polys = [[3, 1, 4], [1, 5, 9], [2, 6, 5]]

    def both(mos, queries, n, z, z_prime=None):
        """the compiled plan's (status, set), which the Python rule must give too"""
        got = host_plan(mos, queries, n, z, 5, 11 if z_prime is not None else None, z_prime)[:2]
        got = got if got[0] != U.PLAN_OK else (U.PLAN_OK, 0)  # a plan that stands names no set
        assert got == U.plan_status(mos, queries, n, z, z_prime), (queries, n, z, z_prime)
        return got

    # kCoincide at z = 0: polynomial 0 alone at one shift (set 0), polynomial 1 at two (set 1): both of its points are 0
    queries = U.with_evals(polys, 0, [(0, 1), (1, 1), (1, w)])
    assert both(U.BDFG21, queries, 3, 0) == (U.PLAN_COINCIDE, 1)
    assert both(U.GWC19, queries, 3, 0) == (U.PLAN_OK, 0)  # Gwc19's sets have one point each
    # kCoincide for two encodings of one shift: different bytes, so two shifts of polynomial 2's set, and one point
    assert w + R < 1 << 256
    queries = U.with_evals(polys, 7, [(0, 1), (1, 1), (1, w2), (2, w), (2, w + R)])
    assert U.claim_of(U.BDFG21, queries).n_sets == 3
    assert both(U.BDFG21, queries, 3, 7) == (U.PLAN_COINCIDE, 2)
    # ... which under Gwc19 are two sets with the same point, and the same r
    status, _, sets, _ = host_plan(U.GWC19, queries, 3, 7, 5)
    assert status == 0 and len(sets) == 4 and sets[2]["polys"] == sets[3]["polys"] == [2]
    assert {k: sets[2][k] for k in ("points", "r", "scalars")} == {k: sets[3][k] for k in ("points", "r", "scalars")}
    assert sets == [{k: st[k] for k in ("polys", "scalars", "points", "r")} for st in U.plan(U.GWC19, queries, 7, 5)]
    # kTooManyPoints at m = n + 1, n = 1 and 2, in a second set
    for n in (1, 2):
        ps = [[5] * n, [7] * n]
        queries = U.with_evals(ps, 7, [(0, 1)] + [(1, U.shift(j)) for j in range(n + 1)])
        assert both(U.BDFG21, queries, n, 7) == (U.PLAN_TOO_MANY_POINTS, 1)
        assert both(U.BDFG21, queries[:-1], n, 7) == (U.PLAN_OK, 0)  # m = n is legal
        assert both(U.GWC19, queries, n, 7) == (U.PLAN_OK, 0)
    # kZeroZ for z' on the first and on the last point of the last set (no other set has either point)
    queries = U.with_evals(polys, 7, [(0, 1), (1, 1), (1, w), (2, w2), (2, U.shift(3)), (2, U.shift(4))])
    assert [st["shifts"] for st in K.bdfg21_query_sets(queries)][2] == [w2, U.shift(3), U.shift(4)]
    assert both(U.BDFG21, queries, 3, 7, 7 * w2 % R) == (U.PLAN_ZERO_Z, 2)
    assert both(U.BDFG21, queries, 3, 7, 7 * U.shift(4) % R) == (U.PLAN_ZERO_Z, 2)
    assert both(U.BDFG21, queries, 3, 7, 7 * w % R) == (U.PLAN_ZERO_Z, 1)
    assert both(U.BDFG21, queries, 3, 7, 7) == (U.PLAN_ZERO_Z, 0)
    assert both(U.BDFG21, queries, 3, 7, 0) == (U.PLAN_OK, 0)  # z' = 0 is legal


def test_what_the_named_entries_are_there_for():
    """the properties the GPU tests rely on, read off the oracle's grouping"""
    c = U.build("np65")
    assert K.bdfg21_query_sets(c.queries)[0]["polys"] == list(range(65)) and c.queries[32][:2] == (32, 1)  # term 33 is query 32
    c = U.build("S65")
    assert [st["polys"] for st in K.gwc19_query_sets(c.queries)] == [[p] for p in range(65)]
    assert [st["polys"] for st in K.bdfg21_query_sets(c.queries)] == [[p] for p in range(65)]
    c = U.build("m5_1000")
    sets = K.bdfg21_query_sets(c.queries)
    assert [len(st["shifts"]) for st in sets] == [5, 2] and c.queries[2][:2] == (0, sets[0]["shifts"][2])
    c = U.build("L33")
    sets = K.bdfg21_query_sets(c.queries)
    assert [st["polys"] for st in sets] == [list(range(16)), list(range(16, 33))] and sets[1]["shifts"] == [1, U.shift(1)]
    c = U.build("zero_job")
    assert not any(c.polys[2]) and all(not any(c.polys[p][1:]) and c.polys[p][0] for p in (0, 1))
    assert [st["polys"] for st in K.gwc19_query_sets(c.queries)] == [[0, 1, 2], [3, 4]]
    assert [q[2] for q in c.queries[:3]] == [c.polys[0][0], c.polys[1][0], 0]
    c = U.build("z_zero")
    assert c.z == 0 and all(q[2] == c.polys[q[0]][0] for q in c.queries)
    c = U.build("rotations")
    w = U.omega16()
    assert pow(w, 16, R) == 1 and pow(w, 8, R) != 1
    sets = K.bdfg21_query_sets(c.queries)
    assert [st["shifts"] for st in sets] == [[1], [1, w], [1, pow(w, -1, R)], [1, w, pow(w, -1, R), w * w % R]]
    assert [len(st["polys"]) for st in sets] == [12, 3, 2, 1]
    assert [len(st["polys"]) for st in K.gwc19_query_sets(c.queries)] == [18, 4, 3, 1]
    for name in ("m_eq_n_2", "m_eq_n_17"):  # a polynomial asked at n points is its own interpolation: that set adds nothing to h
        c = U.build(name)
        st = U.plan(U.BDFG21, c.queries, c.z, 1)[0]
        assert st["polys"] == [0] and st["r"] == c.polys[0]
    # the tiled SRS: one period of distinct points, then the same again
    s = U.srs(U.SECRET_983, 3)
    assert s[:64] == O.g1_to_bytes(O.G1_GEN) and U.mulg(pow(U.SECRET_983, 983 + 2, R)) == s[128:192] and len({s[:64], s[64:128], s[128:]}) == 3


def repeat_case():
    """polynomial 1 asked twice at w, the second time with a wrong evaluation (query 4 repeats query 2)
    -> (polys, z, the list as given, the list without the repeat)"""
    rng = random.Random("kzg-multiopen-repeat")
    polys = [[rng.randrange(R) for _ in range(9)] for _ in range(3)]
    z, w = rng.randrange(1, R), U.shift(1)
    clean = U.with_evals(polys, z, [(0, 1), (1, 1), (1, w), (2, 1)])
    wrong = (1, w, (clean[2][2] + 1) % R)
    return polys, z, clean + [wrong], clean


def test_a_repeated_query_with_a_wrong_second_evaluation_in_the_model():
    """Gwc19 keeps both evaluations (gwc19.rs:142-160), so its set of w holds a wrong one and no proof exists; Bdfg21 keeps
    the first (bdfg21.rs:121-171), so the list proves as the list without the repeat"""
    polys, z, given, clean = repeat_case()
    assert given[4][:2] == given[2][:2] and given[4][2] != given[2][2]
    assert [st["polys"] for st in K.gwc19_query_sets(given)] == [[0, 1, 2], [1, 1]]
    assert K.gwc19_query_sets(given)[1]["evals"] == [given[2][2], given[4][2]]
    assert K.bdfg21_query_sets(given) == K.bdfg21_query_sets(clean)
    # Gwc19: set 1 leaves a remainder, sum v^i (p_i(z w) - e_i) = -v; Bdfg21: none does
    assert U.first_bad_set(U.GWC19, polys, z, given, 3) == 1 and U.first_bad_set(U.GWC19, polys, z, clean, 3) is None
    assert U.first_bad_set(U.BDFG21, polys, z, given, 3) is None
    st = U.plan(U.GWC19, given, z, 3)[1]
    assert (sum(3 ** j * U.horner(polys[1], st["points"][0]) for j in range(2)) - st["r"][0]) % R == R - 3
    # ... and Bdfg21's outputs are those of the list without the repeat, which the oracle's verifier accepts for both lists
    ok_g, ok_b, _, bd = verifies(U.SECRET, polys, z, given, "repeat")
    assert ok_b
    ok_g, ok_b, _, bd_clean = verifies(U.SECRET, polys, z, clean, "repeat")
    assert ok_g and ok_b and bd == bd_clean


@pytest.mark.parametrize("n", U.RANDOM_NS)
def test_the_differential_lists(n):
    """the seeded lists of the GPU differential: the stated count, repeats among them, at most a quarter refused by the plan --
    the compiled one agrees on which -- and every other list proves under the oracle's verifiers"""
    lists = U.random_query_lists(n)
    assert len(lists) == U.RANDOM_LISTS == 12
    assert [q for _, _, q in lists] == [q for _, _, q in U.random_query_lists(n)]  # seeded
    refused = repeats = full = 0
    for i, (polys, z, queries) in enumerate(lists):
        assert 1 <= len(polys) <= 9 and 1 <= len(queries) <= 14 and all(len(p) == n for p in polys)
        repeats += len({q[:2] for q in queries}) != len(queries)
        full += U.claim_of(U.BDFG21, queries).most_points == n
        want = U.plan_status(U.BDFG21, queries, n, z)
        got = host_plan(U.BDFG21, queries, n, z, 5)[:2]
        assert got[0] == want[0] and (got[0] == U.PLAN_OK or got[1] == want[1])
        assert host_plan(U.GWC19, queries, n, z, 5)[0] == U.PLAN_OK
        if want[0] != U.PLAN_OK:
            refused += 1
            continue
        ok_g, ok_b, _, _ = verifies(U.SECRET, polys, z, queries, "differential %d %d" % (n, i))
        assert ok_g and ok_b, (n, i)
    assert 4 * refused <= U.RANDOM_LISTS and repeats
    if n == 5:
        assert full  # some list asks a polynomial at n points
