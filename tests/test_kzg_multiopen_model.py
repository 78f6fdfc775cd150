"""CPU: the expectations and the host-side plan of the KZG multi-open provers (include/snarkv_kzg_multiopen.h).

  * the Python prover of tests/kzg_multiopen_util.py, which the GPU tests hold the device's bytes against, is itself held
    against the verifiers of oracle/kzg.py at every shape those tests use: lhs == [s] rhs.  The expectations are pinned by
    the existing oracle, not by the code under test.
  * the plan of csrc/kzg_multiopen_plan.h, compiled alone (tests/hosttest/hosttest_kzg_open.cpp), equals the util's number
    for number: set order, polynomial order, the scalars of the linear combinations, the coefficients of r, and after z' the
    scalars of L, its constant and Z_1(z').
  * snarkv_kzg_multiopen_sets agrees with gwc19_query_sets / bdfg21_query_sets on random query lists with repeated
    (polynomial, shift) pairs.

("three points at n = 3, alone": W is the identity there, W' is not -- L = q - q(z') -- and the util says so.  The shape
where every output of both schemes is the identity is "constants, n = 1".)"""
import ctypes
import importlib.util
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import kzg as K  # noqa: E402
import kzg_multiopen_util as U  # noqa: E402

R = O.R
SECRET = 0x5EC2E7_0F_7AE_542
_LIBS = {}
ZERO64 = b"\x00" * 64


def host_lib(curve="bn254"):
    if curve not in _LIBS:
        spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        lib = ctypes.CDLL(b.build_hosttest("kzg_open", curve))
        lib.hko_curve.restype = ctypes.c_char_p
        lib.hko_sets.restype = ctypes.c_long
        lib.hko_sets.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.hko_plan.restype = ctypes.c_size_t
        lib.hko_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
        assert lib.hko_curve() == curve.encode()
        _LIBS[curve] = lib
    return _LIBS[curve]


def all_cases():
    """name -> (polys, z, queries): every shape of tests/test_gpu_kzg_multiopen.py"""
    rng = random.Random("kzg-multiopen-cases")
    cases = {"standard plonk, n = %d" % n: U.standard_plonk_instance(rng, n) for n in (4, 257, 1000)}
    cases.update(U.set_shape_cases(rng))
    return cases


CASES = all_cases()


def _pt(b):
    return O.g1_from_bytes(b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_expected_points_satisfy_the_oracle_verifiers(name):
    polys, z, queries = CASES[name]
    rng = random.Random("verify " + name)
    v, u, mu, gamma = (rng.randrange(1, R) for _ in range(4))
    cms = [K.Msm.base(c) for c in U.commitments(SECRET, polys)]
    ws = U.gwc19_prove(SECRET, polys, z, queries, v)
    assert len(ws) == len(K.gwc19_query_sets(queries))
    lhs, rhs = K.gwc19_verify(O.G1_GEN, cms, z, queries, v, [_pt(w) for w in ws], u)
    assert lhs == O.g1_mul(rhs, SECRET) if rhs is not None else lhs is None
    w, z_prime, w_prime = U.bdfg21_prove(SECRET, polys, z, queries, mu, gamma, U.draw_from(name))
    lhs, rhs = K.bdfg21_verify(O.G1_GEN, cms, z, queries, mu, gamma, _pt(w), z_prime, _pt(w_prime))
    assert lhs == O.g1_mul(rhs, SECRET) if rhs is not None else lhs is None
    if name == "three points at n = 3, alone":
        assert w == ZERO64 and w_prime != ZERO64
    if name == "constants, n = 1":
        assert ws == [ZERO64] * 2 and w == ZERO64 and w_prime == ZERO64
    # a wrong evaluation does not verify: the expectation is not vacuous
    bad = [(queries[0][0], queries[0][1], (queries[0][2] + 1) % R)] + queries[1:]
    lhs, rhs = K.gwc19_verify(O.G1_GEN, cms, z, bad, v, [_pt(w) for w in ws], u)
    assert lhs != (O.g1_mul(rhs, SECRET) if rhs is not None else None)


def _records(buf, count):
    return [int.from_bytes(buf[32 * i:32 * i + 32], "little") for i in range(count)]


def host_plan(mos, queries, n, z, c, gamma=None, z_prime=None, curve="bn254"):
    """the plan of the C++ header as the util shapes it: (status, bad set, sets, L or None)"""
    lib = host_lib(curve)
    qp = np.array([q[0] for q in queries], dtype=np.uint32)
    qs = b"".join(int(q[1]).to_bytes(32, "little") for q in queries)
    qe = b"".join(int(q[2]).to_bytes(32, "little") for q in queries)
    cap = 16 + 8 * len(queries)
    out = ctypes.create_string_buffer(32 * cap)
    status, bad = ctypes.c_int(-1), ctypes.c_size_t(0)
    fe = lambda x: None if x is None else int(x).to_bytes(32, "little")  # noqa: E731
    used = lib.hko_plan(mos, qp.ctypes.data_as(ctypes.c_void_p), qs, qe, len(queries), n, fe(z), fe(c), fe(gamma), fe(z_prime), out, cap,
                        ctypes.byref(status), ctypes.byref(bad))
    if status.value != 0:
        return status.value, bad.value, None, None
    assert used <= cap
    rec = _records(out.raw, used)
    pos, sets = 1, []
    for _ in range(rec[0]):
        m, npolys = rec[pos], rec[pos + 1]
        pos += 2
        st = {"polys": rec[pos:pos + npolys], "scalars": rec[pos + npolys:pos + 2 * npolys]}
        pos += 2 * npolys
        st["points"], st["r"] = rec[pos:pos + m], rec[pos + m:pos + 2 * m]
        pos += 2 * m
        sets.append(st)
    big_l = None
    if gamma is not None:
        t = rec[pos]
        big_l = {"idx": rec[pos + 1:pos + 1 + t], "scalars": rec[pos + 1 + t:pos + 1 + 2 * t], "constant": rec[pos + 1 + 2 * t],
                 "z1": rec[pos + 2 + 2 * t]}
        pos += 3 + 2 * t
    assert pos == used
    return 0, bad.value, sets, big_l


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_plan_equals_the_python_plan_number_for_number(name):
    polys, z, queries = CASES[name]
    n = len(polys[0])
    rng = random.Random("plan " + name)
    v, mu, gamma, z_prime = (rng.randrange(1, R) for _ in range(4))
    for mos, c in ((U.GWC19, v), (U.BDFG21, mu)):
        want = U.plan(mos, queries, z, c)
        status, _, sets, big_l = host_plan(mos, queries, n, z, c, gamma if mos == U.BDFG21 else None, z_prime if mos == U.BDFG21 else None)
        assert status == 0
        assert sets == [{k: st[k] for k in ("polys", "scalars", "points", "r")} for st in want], (name, mos)
        if mos == U.BDFG21:
            assert big_l == U.plan_finish(want, gamma, z_prime), name


def test_the_plan_refuses_what_the_header_says():
    w1 = 12345
    polys = [[3, 1, 4], [1, 5, 9]]
    queries = U.with_evals(polys, 7, [(0, 1), (0, w1), (1, 1)])
    assert host_plan(U.BDFG21, queries, 3, 0, 5)[:2] == (2, 0)  # kCoincide: z = 0 puts both points of set 0 at 0
    assert host_plan(U.GWC19, queries, 3, 0, 5)[0] == 0        # ... Gwc19's sets have one point each
    assert host_plan(U.BDFG21, queries, 1, 7, 5)[:2] == (3, 0)  # kTooManyPoints
    assert host_plan(U.BDFG21, queries, 3, 7, 5, 11, 7)[:2] == (4, 0)  # kZeroZ: z' = z * 1 is a point of sets 0 and 1
    assert host_plan(U.BDFG21, queries, 3, 7, 5, 11, 7 * w1 % R)[:2] == (4, 0)
    assert host_plan(2, queries, 3, 7, 5)[0] == 1  # kBadMos
    # the plan is scalar-field arithmetic only: the pallas build of the same header runs the same rule over its own field
    assert host_lib("pallas").hko_selftest() == 0 and host_lib("bn254").hko_selftest() == 0


def test_set_counts_match_the_oracle_on_random_query_lists():
    from snark_verifier_amd import kzg_multiopen as KM

    rnd = random.Random("kzg-set-counts")
    for _ in range(40):
        queries = [(rnd.randrange(6), rnd.choice([1, 5, 7, 11, R - 1]), rnd.randrange(R)) for _ in range(rnd.randrange(1, 16))]
        assert KM.n_sets(KM.MOS_GWC19, queries) == len(K.gwc19_query_sets(queries)), queries
        assert KM.n_sets(KM.MOS_BDFG21, queries) == len(K.bdfg21_query_sets(queries)), queries
    a = KM.api()
    out = ctypes.c_size_t(77)
    qp, qs = (ctypes.c_uint32 * 1)(0), (1).to_bytes(32, "little")
    assert a.kzg_multiopen_sets(2, qp, qs, 1, ctypes.byref(out)) == -5 and out.value == 77  # an unknown scheme
    assert a.kzg_multiopen_sets(0, qp, qs, 1, None) == -5 and a.kzg_multiopen_sets(0, None, qs, 1, ctypes.byref(out)) == -5
    assert a.kzg_multiopen_sets(1, None, None, 0, ctypes.byref(out)) == 0 and out.value == 0
