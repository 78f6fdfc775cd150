"""CPU: the catalogue of query shapes in tests/multiopen_util.py is what it says, before any kernel runs.  For every entry on
BN254 and pallas the oracle's prover (oracle/ipa.py::bgh19_create_proof) gives a proof of 64 k + 32 S + 160 bytes that the
oracle's verifier accepts and `ipa_decide` decides; `bdfg21_query_sets` returns the set count, the largest set and the most
points that the entry claims; and the prover's own grouping (csrc/ipa_multiopen_sets.h through
tests/hosttest/hosttest_poly.cpp::hp_query_sets) is the oracle's: set order, polynomial order, evaluation order."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiopen_util as U  # noqa: E402

CURVE_NAMES = ["bn254", "pallas"]


@pytest.fixture(scope="module")
def host_libs():
    from test_poly_scan_model import host_lib

    return {curve: host_lib(curve) for curve in CURVE_NAMES}


def test_the_catalogue_is_laid_out_around_the_pass_length():
    from snark_verifier_amd import poly

    assert poly.LINCOMB_TERMS == U.TERMS == 32
    sh = U.SHAPES
    assert [sh[n].largest_set for n in ("np32", "np33", "np65")] == [U.TERMS, U.TERMS + 1, 2 * U.TERMS + 1]
    # f's combination has S terms, p's S + 1
    assert [sh[n].n_sets for n in ("S31", "S32", "S33")] == [U.TERMS - 1, U.TERMS, U.TERMS + 1]
    for k in (1, 2, 3):
        assert sh["m_eq_n_k%d" % k].k == k and sh["m_eq_n_k%d" % k].most_points == 1 << k
    assert all(s.k <= U.MAX_K and s.reaches for s in sh.values())
    assert set(U.DEV_FORM) <= set(sh)


@pytest.mark.parametrize("name", list(U.SHAPES))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_oracle_proves_verifies_and_decides(curve, name):
    c = U.build(curve, name)
    proof = c.oracle()
    assert len(proof) == U.proof_len(c.k, c.n_sets) == 64 * c.k + 32 * U.SHAPES[name].n_sets + 160
    acc = c.verify(proof)
    assert len(acc[0]) == c.k
    assert c.decides_on_host(acc)
    # one bit of the first q_i(x_3) flipped: the verifier or the decider refuses
    flipped = proof[:32] + bytes([proof[32] ^ 1]) + proof[33:]
    try:
        bad = c.verify(flipped)
    except (U.I.IpaError, U.T.TranscriptError, AssertionError, ValueError):
        bad = None
    assert bad is None or not c.decides_on_host(bad)


@pytest.mark.parametrize("name", list(U.SHAPES))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_grouping_is_what_the_entry_claims(curve, name):
    c, sh = U.build(curve, name), U.SHAPES[name]
    assert U.largest(c.sets) == (sh.n_sets, sh.largest_set, sh.most_points)
    assert sh.most_points <= c.n  # within `st.shifts.size() > n`
    queried = {q[0] for q in c.queries}
    assert max(queried) < c.n_polys
    assert sorted(p for st in c.sets for p in st["polys"]) == sorted(queried)


def _host_sets(lib, queries):
    qp = np.array([q[0] for q in queries], dtype=np.uint32)
    qs = b"".join(U.fe(q[1]) for q in queries)
    out = np.zeros(8192, dtype=np.uint32)  # np40_two_sets, the largest, takes 195 words
    used = lib.hp_query_sets(qp.ctypes.data_as(ctypes.c_void_p), qs, len(queries), out.ctypes.data_as(ctypes.c_void_p), len(out))
    assert used <= len(out)
    flat, got, pos = [int(v) for v in out[:used]], [], 1
    for _ in range(flat[0]):
        m, npolys = flat[pos], flat[pos + 1]
        pos += 2
        shifts = [queries[q][1] for q in flat[pos:pos + m]]
        pos += m
        polys = flat[pos:pos + npolys]
        pos += npolys
        evals = [[queries[q][2] for q in flat[pos + m * j:pos + m * (j + 1)]] for j in range(npolys)]
        pos += m * npolys
        got.append({"shifts": shifts, "polys": polys, "evals": evals})
    assert pos == used
    return got


@pytest.mark.parametrize("name", list(U.SHAPES))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_host_grouping_matches_the_oracle(host_libs, curve, name):
    c = U.build(curve, name)
    assert _host_sets(host_libs[curve], c.queries) == c.sets


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_what_the_named_entries_are_there_for(curve):
    """the properties the GPU tests rely on, read off the oracle's grouping"""
    c = U.build(curve, "np40_two_sets")
    assert [len(st["polys"]) for st in c.sets] == [40, 35] and c.sets[0]["polys"] == list(range(40))
    # set 1: polynomial 74 first, its order (1, w); the term of x_1^33 is polynomial 73, asked as (w, 1)
    one = c.sets[1]
    assert one["polys"] == list(range(74, 39, -1)) and one["shifts"][0] == 1
    term33 = list(reversed(one["polys"]))[33]
    asked = [q[1] for q in c.queries if q[0] == term33]
    assert term33 == 73 and asked == one["shifts"][::-1]
    assert one["evals"][one["polys"].index(73)] == [c.eval_at(73, s) for s in one["shifts"]]

    c = U.build(curve, "np40_regrouped")
    assert [st["polys"] for st in c.sets] == [list(range(35)), list(range(35, 40))]
    assert c.sets[0]["evals"][1] == [c.queries[1][2], c.queries[-2][2]] and c.queries[-2][:2] == (1, c.sets[0]["shifts"][1])

    c = U.build(curve, "first_set_by_last_poly")
    assert [st["polys"] for st in c.sets] == [[7, 4], [6, 2, 0], [1]]
    assert c.sets[0]["evals"][1] == [c.eval_at(4, s) for s in c.sets[0]["shifts"]]

    c = U.build(curve, "dup_first_wins")
    first, second = c.queries[U.DUP_FIRST], c.queries[U.DUP_SECOND]
    assert first[:2] == second[:2] and first[2] == c.eval_at(*first[:2]) != second[2]
    assert c.sets[1]["polys"] == [1] and c.sets[1]["evals"] == [[c.queries[1][2], first[2]]]

    c = U.build(curve, "rotations")
    w = U.ntt_util.omega(curve, 4)
    assert pow(w, 16, c.r) == 1 and pow(w, 8, c.r) != 1
    assert [st["shifts"] for st in c.sets] == [[1], [1, w], [1, pow(w, -1, c.r)], [1, w, pow(w, -1, c.r), w * w % c.r]]
    assert [len(st["polys"]) for st in c.sets] == [12, 3, 2, 1]

    c = U.build(curve, "x_zero")
    assert c.x == 0 and all(q[2] == c.polys[q[0]][0] for q in c.queries)
    c = U.build(curve, "zero_polys")
    assert not any(v for p in c.polys for v in p) and all(c.blinds) and not any(q[2] for q in c.queries)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_differential_lists(host_libs, curve, k):
    """the seeded lists of the GPU differential: the stated count, each within the prover's limit, grouped alike on both sides"""
    lists = U.random_pair_lists(curve, k)
    assert len(lists) == U.RANDOM_LISTS == 12
    assert lists == U.random_pair_lists(curve, k)  # seeded
    repeats = 0
    for n_polys, pairs in lists:
        assert 1 <= n_polys <= 9 and 1 <= len(pairs) <= 14
        queries = [(p, s, 1000 * i + 7) for i, (p, s) in enumerate(pairs)]
        with U.on_curve(curve):
            sets = U.K.bdfg21_query_sets(queries)
        assert max(len(st["shifts"]) for st in sets) <= 1 << k
        assert _host_sets(host_libs[curve], queries) == sets
        repeats += len(pairs) != len(set(pairs))
    assert repeats  # some list repeats a (polynomial, shift)
