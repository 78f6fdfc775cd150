"""CPU: the C ABI of the resident-polynomial calls and of the Bgh19 multi-open prover (include/snarkv_poly.h,
include/snarkv_ipa_multiopen.h): the headers are strict C99, both device libraries export every declared name and only
their own, the ctypes tables of snark_verifier_amd.poly and snark_verifier_amd.ipa_multiopen list exactly those names and
share none with the other tables, bad arguments are refused with the documented codes before any device work, and the
prover's query-set grouping (csrc/ipa_multiopen_sets.h, through tests/hosttest/hosttest_poly.cpp) is that of
oracle/kzg.py::bdfg21_query_sets: set order, polynomial order, evaluation order."""
import ctypes
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
POLY_HDR = os.path.join(INC, "snarkv_poly.h")
MO_HDR = os.path.join(INC, "snarkv_ipa_multiopen.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402


def test_headers_are_strict_c99():
    for h in (POLY_HDR, MO_HDR):
        AU.assert_strict_c99(h)


def test_both_libraries_export_every_declared_name_and_the_tables_list_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_multiopen, poly
    from snark_verifier_amd import pallas as PL

    want_poly = sorted(p + n for p in ("snarkv_", "snarkv_pallas_") for n in ("poly_lincomb_dev", "poly_eval_dev", "poly_div_linear_dev"))
    want_mo = sorted(["bn254_ipa_multiopen_create_proof", "pallas_ipa_multiopen_create_proof", "snarkv_ipa_multiopen_create_proof",
                      "snarkv_ipa_multiopen_create_proof_dev", "snarkv_pallas_ipa_multiopen_create_proof",
                      "snarkv_pallas_ipa_multiopen_create_proof_dev"])
    assert AU.declared(POLY_HDR) == want_poly == sorted(poly.SIGNATURES)
    assert AU.declared(MO_HDR) == want_mo == sorted(ipa_multiopen.SIGNATURES)
    assert not set(want_poly) & AU.other_tables(poly) and not set(want_mo) & AU.other_tables(ipa_multiopen)
    bn, pa = sv.load_library(), PL.load_library()
    for name in want_poly + want_mo:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("create_proof", "create_proof_dev", "create_proof_default", "proof_bytes", "pack_queries"):
        assert callable(getattr(sv.ipa_multiopen, fn))
    for fn in ("lincomb_dev", "eval_dev", "div_linear_dev"):
        assert callable(getattr(sv.poly, fn))
    assert sv.ipa_multiopen.proof_bytes(10, 3) == 64 * 10 + 32 * 3 + 160


def test_multiopen_refuses_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_multiopen as MO

    for pallas in (False, True):
        a = MO.api(pallas)
        b32, b64, polys = b"\x00" * 32, b"\x01" * 64, b"\x00" * (32 * 8 * 2)
        proof, xi, u = ctypes.create_string_buffer(b"\xaa" * 512, 512), ctypes.create_string_buffer(96), ctypes.create_string_buffer(64)
        plen = ctypes.c_size_t(7)
        ctx = AU.FakeCtx(device=0)
        whole, shard = AU.FakeKey(device=0, k=3, first=0, count=8), AU.FakeKey(device=0, k=3, first=4, count=4)
        pc, pw, ps = ctypes.addressof(ctx), ctypes.addressof(whole), ctypes.addressof(shard)
        one = (1).to_bytes(32, "little")
        two = (2).to_bytes(32, "little")
        qp = (ctypes.c_uint32 * 3)(0, 1, 1)

        def call(fn=a.ipa_multiopen_create_proof, c=pc, dk=pw, h=b64, s=b64, p=polys, n=8, npolys=2, bl=b32 * 2, x=b32, q=qp,
                 qs=one + one + two, qe=b32 * 3, nq=3, fb=b32, pbar=polys[:256], omb=b32, ab=None, ablen=0, out=proof, cap=512,
                 ln=ctypes.byref(plen), xx=xi, uu=u):
            return fn(c, dk, h, s, p, n, npolys, bl, x, q, qs, qe, nq, fb, pbar, omb, ab, ablen, out, cap, ln, xx, uu)

        # null arguments; s is required as h is: the scheme is always zero-knowledge
        for name in ("c", "dk", "h", "s", "p", "bl", "x", "q", "qs", "qe", "fb", "pbar", "omb", "out", "ln", "xx", "uu"):
            assert call(**{name: None}) == sv.SNARKV_ERR_ARG, name
        assert call(ablen=5) == sv.SNARKV_ERR_ARG  # absorbed bytes announced, none given
        assert call(fn=a.ipa_multiopen_create_proof_dev, p=None) == sv.SNARKV_ERR_ARG
        # the key and n: a shard, n that is not the key's 2^k, a context on another device
        assert call(dk=ps) == sv.SNARKV_ERR_LENGTH and plen.value == 0
        assert call(n=4) == sv.SNARKV_ERR_LENGTH
        other = AU.FakeCtx(device=1)
        assert call(c=ctypes.addressof(other)) == sv.SNARKV_ERR_ARG
        # nothing to open
        assert call(npolys=0) == sv.SNARKV_ERR_EMPTY and call(nq=0) == sv.SNARKV_ERR_EMPTY
        # a query names a polynomial that is not there
        assert call(q=(ctypes.c_uint32 * 3)(0, 2, 1)) == sv.SNARKV_ERR_ARG
        assert "polynomial 2 of 2" in a.last_error()
        # proof_cap one byte short: two sets ({1}, {1, 2}) at k = 3; the needed length comes back, nothing else is written
        need = MO.proof_bytes(3, 2)
        assert call(cap=need - 1) == sv.SNARKV_ERR_LENGTH and plen.value == need == 64 * 3 + 32 * 2 + 160
        assert call(cap=MO.proof_bytes(3, 1) - 1, nq=2) == sv.SNARKV_ERR_LENGTH and plen.value == MO.proof_bytes(3, 1)
        assert proof.raw == b"\xaa" * 512


def test_poly_calls_refuse_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import poly as P

    for pallas in (False, True):
        a = P.api(pallas)
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        base = 0x10000  # device addresses are only compared here, never followed
        idx = (ctypes.c_uint32 * 2)(0, 1)
        sc = b"\x00" * 64
        n = 8
        out = base + 32 * n * 2
        assert a.poly_lincomb_dev(None, base, n, 2, idx, sc, 2, out) == sv.SNARKV_ERR_ARG
        assert a.poly_lincomb_dev(pc, None, n, 2, idx, sc, 2, out) == sv.SNARKV_ERR_ARG
        assert a.poly_lincomb_dev(pc, base, n, 2, None, sc, 2, out) == sv.SNARKV_ERR_ARG
        assert a.poly_lincomb_dev(pc, base, n, 2, idx, None, 2, out) == sv.SNARKV_ERR_ARG
        assert a.poly_lincomb_dev(pc, base + 8, n, 2, idx, sc, 2, out) == sv.SNARKV_ERR_ARG  # 16-byte alignment
        assert a.poly_lincomb_dev(pc, base, 0, 2, idx, sc, 2, out) == sv.SNARKV_ERR_EMPTY
        assert a.poly_lincomb_dev(pc, base, n, 2, idx, sc, 0, out) == sv.SNARKV_ERR_EMPTY
        assert a.poly_lincomb_dev(pc, base, (1 << 30) + 1, 2, idx, sc, 2, out) == sv.SNARKV_ERR_LENGTH
        assert a.poly_lincomb_dev(pc, base, n, 2, (ctypes.c_uint32 * 2)(0, 2), sc, 2, out) == sv.SNARKV_ERR_ARG  # index >= n_polys
        assert "index 2" in (a.lib.snarkv_pallas_last_error() if pallas else a.lib.snarkv_last_error()).decode()
        assert a.poly_lincomb_dev(pc, base, n, 2, idx, sc, 2, base + 32 * n) == sv.SNARKV_ERR_ARG  # out is polynomial 1
        assert a.poly_lincomb_dev(pc, base, n, 2, idx, sc, 2, base + 32 * (2 * n - 1)) == sv.SNARKV_ERR_ARG  # ... or its last coefficient
        point, res = base + 0x8000, base + 0x8020
        assert a.poly_eval_dev(None, base, n, point, res) == sv.SNARKV_ERR_ARG
        assert a.poly_eval_dev(pc, base, n, None, res) == sv.SNARKV_ERR_ARG
        assert a.poly_eval_dev(pc, base, n, point, None) == sv.SNARKV_ERR_ARG
        assert a.poly_eval_dev(pc, base, 0, point, res) == sv.SNARKV_ERR_EMPTY
        assert a.poly_eval_dev(pc, base, (1 << 30) + 1, point, res) == sv.SNARKV_ERR_LENGTH
        quot = base + 0x4000
        assert a.poly_div_linear_dev(None, base, n, point, quot, res) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, n, point, None, res) == sv.SNARKV_ERR_ARG  # n > 1 has a quotient
        assert a.poly_div_linear_dev(pc, base, n, point, quot, None) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, 0, point, quot, res) == sv.SNARKV_ERR_EMPTY
        # the header's promise: the quotient may not overlap the coefficients, at either end, nor may the remainder
        assert a.poly_div_linear_dev(pc, base, n, point, base, res) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, n, point, base + 32 * (n - 1), res) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, n, point, base - 32 * (n - 2), res) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, n, point, quot, base + 32) == sv.SNARKV_ERR_ARG
        assert a.poly_div_linear_dev(pc, base, n, point, quot, quot + 32) == sv.SNARKV_ERR_ARG


def multiopen_queries(w, w2, evals=None):
    """the query list of the multi-open tests: polynomials 0-2 at shift 1, 3 at (1, w), 4 at (w, 1) -- the other order, so that
    3 and 4 land in one set with 4's evaluations re-ordered -- and 5 at (1, w, w').  evals: (poly, shift) -> evaluation"""
    ev = evals if evals is not None else (lambda poly, shift: 1000 * poly + shift % 1000)
    pairs = [(0, 1), (1, 1), (2, 1), (3, 1), (3, w), (4, w), (4, 1), (5, 1), (5, w), (5, w2)]
    return [(p, s, ev(p, s)) for p, s in pairs]


def test_grouping_matches_the_oracle():
    import kzg as K
    from test_poly_scan_model import host_lib

    rnd = random.Random("multiopen-grouping")
    lib = host_lib("bn254")
    cases = [multiopen_queries(5, 7), multiopen_queries(5, 7)[::-1], [(0, 1, 9), (0, 1, 10), (1, 1, 3)]]
    for _ in range(20):  # random lists over few polynomials and shifts, repeats included
        cases.append([(rnd.randrange(5), rnd.choice([1, 5, 7, 11]), rnd.randrange(1 << 200)) for _ in range(rnd.randrange(1, 14))])
    for queries in cases:
        want = K.bdfg21_query_sets(queries)
        qp = np.array([q[0] for q in queries], dtype=np.uint32)
        qs = b"".join(int(q[1]).to_bytes(32, "little") for q in queries)
        out = np.zeros(4096, dtype=np.uint32)
        used = lib.hp_query_sets(qp.ctypes.data_as(ctypes.c_void_p), qs, len(queries), out.ctypes.data_as(ctypes.c_void_p), len(out))
        assert used <= len(out)
        flat, got = [int(v) for v in out[:used]], []
        pos = 1
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
        assert got == want, queries
    first = K.bdfg21_query_sets(cases[0])
    assert [st["polys"] for st in first] == [[0, 1, 2], [3, 4], [5]]
    assert first[1]["evals"][1] == [4001, 4005]  # polynomial 4's evaluations in the set's order (1, w)
