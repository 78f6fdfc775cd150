"""GPU: the Bgh19 multi-open prover (csrc/ipa_multiopen.hip) at the query shapes of tests/multiopen_util.py::SHAPES, each
there for a line of the prover or of csrc/poly.hip: sets of more than 32 polynomials, more than 31 sets, up to n points per
set, the grouping's edge rules, x = 0, zero polynomials.  Byte for byte against oracle/ipa.py::bgh19_create_proof on BN254
and pallas, the accumulator against the oracle's verifier and the device's decide; the device-resident form between guards;
a context whose first call is the prover; wrong evaluations past term 31 and in two sets at once; the refusals of too many
points, coinciding points and an f at infinity; and a seeded differential over random query lists."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiopen_util as U  # noqa: E402
from test_gpu_ipa_create import INFINITY_TEXT  # noqa: E402
from test_gpu_ipa_multiopen import MISMATCH_TEXT  # noqa: E402

pytestmark = pytest.mark.gpu
CURVE_NAMES = ["bn254", "pallas"]
GUARD = 4096


@pytest.fixture(scope="module")
def MO():
    from snark_verifier_amd import ipa_multiopen

    return ipa_multiopen


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_of(gpu_ctx, pctx):
    """curve name -> its context; the deciding keys the shared cases made on them are closed before the contexts are"""
    yield lambda curve: pctx if curve == "pallas" else gpu_ctx
    U.close_all()


def _new_context(curve):
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    return PL.PallasContext(0) if curve == "pallas" else sv.Context(0)


def _check_parity(MO, ctx, c, queries=None):
    want = c.oracle()
    proof, acc = c.device(MO, ctx, queries=queries)
    assert len(proof) == MO.proof_bytes(c.k, c.n_sets) == 64 * c.k + 32 * c.n_sets + 160
    assert proof == want
    # the oracle's verifier reads the device's bytes back and ends at the same accumulator, which the device decides
    c.commit_on(ctx)
    assert c.verify(proof) == (acc[0], acc[1])
    assert c.decides(ctx, acc)


@pytest.mark.parametrize("name", list(U.SHAPES))
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_parity_at_every_shape(MO, ctx_of, curve, name):
    ctx = ctx_of(curve)
    c = U.build(curve, name)
    assert U.largest(c.sets) == U.SHAPES[name][3:6]
    _check_parity(MO, ctx, c)


@pytest.mark.parametrize("name", U.DEV_FORM)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_device_resident_form(MO, ctx_of, curve, name):
    """the same bytes from polynomials and p_bar in device memory, both unchanged afterwards, nothing written around them"""
    import torch

    ctx = ctx_of(curve)
    c = U.build(curve, name)
    pb, bar = c.polys_bytes(), c.p_bar_bytes()
    guarded = b"\xaa" * GUARD + pb + b"\xaa" * GUARD
    d_polys = torch.frombuffer(bytearray(guarded), dtype=torch.uint8).cuda()
    d_bar = torch.frombuffer(bytearray(bar), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert (d_polys.data_ptr() + GUARD) % 16 == 0
    proof, acc = c.device_dev(MO, ctx, d_polys.data_ptr() + GUARD, d_bar.data_ptr())
    assert proof == c.oracle()
    assert (proof, acc) == c.device(MO, ctx)
    torch.cuda.synchronize()
    assert bytes(d_polys.cpu().numpy()) == guarded
    assert bytes(d_bar.cpu().numpy()) == bar


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_first_call_on_a_fresh_context(MO, curve):
    """SLOT_POLY is allocated inside the call that takes the second pass, then grows for n = 16 on the same context"""
    ctx = _new_context(curve)
    try:
        for name in ("np33", "rotations"):
            c = U.build(curve, name)
            try:
                assert c.device(MO, ctx)[0] == c.oracle(), name
            finally:
                c.close(ctx)
    finally:
        ctx.close()


# ---- the raw C call on buffers filled with 0xAA ----------------------------------------------------------------------------
def _raw_call(MO, ctx, c, queries=None):
    """-> (code, proof_len, the three output buffers afterwards, the api)"""
    a = MO.api(c.curve == "pallas")
    queries = c.queries if queries is None else queries
    full = MO.proof_bytes(c.k, len(queries))
    bufs = [ctypes.create_string_buffer(b"\xaa" * m, m) for m in (full, 32 * c.k, 64)]
    plen = ctypes.c_size_t(7)
    pt = lambda q: U.fe(q[0]) + U.fe(q[1])  # noqa: E731
    qp, qs, qe, nq = MO.pack_queries(queries)
    rc = a.ipa_multiopen_create_proof(ctx._h, c.dk(ctx)._h, pt(c.pk.h), pt(c.pk.s), c.polys_bytes(), c.n, c.n_polys,
                                      b"".join(U.fe(v) for v in c.blinds), U.fe(c.x), qp, qs, qe, nq, U.fe(c.f_blind), c.p_bar_bytes(),
                                      U.fe(c.omega_bar), None, 0, bufs[0], full, ctypes.byref(plen), bufs[1], bufs[2])
    return rc, plen.value, [b.raw for b in bufs], a


def _refused(MO, ctx, c, code, texts, queries=None):
    rc, plen, bufs, a = _raw_call(MO, ctx, c, queries)
    assert rc == code and plen == 0, (rc, a.last_error())
    for text in texts:
        assert text in a.last_error(), (text, a.last_error())
    assert all(b == b"\xaa" * len(b) for b in bufs)


def _query_of(c, poly, shift):
    at, = [i for i, q in enumerate(c.queries) if q[:2] == (poly, shift)]
    return at


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_wrong_evaluations_past_term_31(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.build(curve, "np40_two_sets")
    w = c.sets[1]["shifts"][1]
    # set 0 = polynomials 0..39, the term of x_1^j is polynomial 39 - j: the 33rd term (the first of the second pass) and the
    # term of x_1^33; set 1 = 74..40 reversed: the term of x_1^33 is polynomial 73, whose evaluations were re-ordered
    for at, bad_set in ((_query_of(c, 39 - 32, 1), 0), (_query_of(c, 39 - 33, 1), 0), (_query_of(c, 73, w), 1), (_query_of(c, 73, 1), 1)):
        bad = c.with_eval({at: c.queries[at][2] + 1})
        _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set %d)" % bad_set], bad)
        assert c.device(MO, ctx)[0] == c.oracle()  # the next correct call on the same context
    # the first set of `np40_regrouped` is polynomials 0..34 at (1, w): the term of x_1^33 is polynomial 1, its evaluation at
    # w the query before the last
    c = U.build(curve, "np40_regrouped")
    at = _query_of(c, 34 - 33, w)
    assert at == len(c.queries) - 2
    _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set 0)"], c.with_eval({at: c.queries[at][2] + 1}))
    assert c.device(MO, ctx)[0] == c.oracle()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_a_wrong_evaluation_at_the_third_of_five_points(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.build(curve, "m5")
    at = _query_of(c, 0, c.sets[0]["shifts"][2])
    _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set 0)"], c.with_eval({at: c.queries[at][2] + 1}))
    assert c.device(MO, ctx)[0] == c.oracle()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_of_a_repeated_query_the_first_evaluation_counts(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.build(curve, "dup_first_wins")
    first, second = c.queries[U.DUP_FIRST], c.queries[U.DUP_SECOND]
    assert first[:2] == second[:2] and first[2] != second[2]
    _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set 1)"], c.with_eval({U.DUP_FIRST: first[2] + 1}))
    # the second alone changed, to yet another value and to the first's wrong one: unused.  The oracle's prover reads no
    # evaluation at all (it evaluates q itself), so its bytes are those of the unchanged list.
    for ev in (second[2] + 5, first[2] + 1):
        _check_parity(MO, ctx, c, c.with_eval({U.DUP_SECOND: ev}))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_two_bad_sets_name_the_lower(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.build(curve, "rotations")
    in1, in3 = _query_of(c, 13, c.sets[1]["shifts"][1]), _query_of(c, 17, c.sets[3]["shifts"][2])
    bad = c.with_eval({in1: c.queries[in1][2] + 1, in3: c.queries[in3][2] + 1})
    _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set 1)"], bad)
    _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, [MISMATCH_TEXT, "set 3)"], c.with_eval({in3: c.queries[in3][2] + 1}))
    assert c.device(MO, ctx)[0] == c.oracle()


# ---- refusals: each returns with the outputs at 0xAA and proof_len 0 ----------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_more_points_than_coefficients(MO, ctx_of, curve, k):
    import snark_verifier_amd as sv

    ctx, n = ctx_of(curve), 1 << k
    c = U.ShapeCase(curve, k, 1, [(0, U.shift(curve, j)) for j in range(n + 1)], "n-plus-one")
    try:
        assert U.largest(c.sets) == (1, 1, n + 1)
        _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, ["queried at %d points" % (n + 1), "%d coefficients" % n])
    finally:
        c.close()
    ok = U.build(curve, "m_eq_n_k%d" % k)  # n points are allowed, on the same context
    assert ok.device(MO, ctx)[0] == ok.oracle()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_two_encodings_of_one_shift_coincide(MO, ctx_of, curve):
    """s and s + r are different bytes, so the grouping sees two shifts, and one point"""
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    s = U.shift(curve, 1)
    c = U.ShapeCase(curve, 3, 2, [(0, 1), (1, s), (1, s)], "alias")
    assert s + c.r < 1 << 256
    bad = [(q[0], U.fe(q[1]), q[2]) for q in c.queries]
    bad[2] = (1, U.fe(s + c.r), bad[2][2])
    try:
        _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, ["two points of query set 1 coincide"], bad)
        assert c.device(MO, ctx)[0] == c.oracle()
        ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
        try:
            _refused(MO, ctx, c, sv.SNARKV_ERR_ENCODING, ["not canonical"], bad)
        finally:
            ctx.set_flags(0)
        _check_parity(MO, ctx, c)  # the repeat in canonical bytes is a duplicate query, and fine
    finally:
        c.close()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_x_zero_with_a_two_shift_set(MO, ctx_of, curve):
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.ShapeCase(curve, 3, 2, [(0, 1), (1, 1), (1, U.shift(curve, 1))], "x-zero-two-shifts", x=0)
    try:
        _refused(MO, ctx, c, sv.SNARKV_ERR_ARG, ["two points of query set 1 coincide"])
    finally:
        c.close()
    ok = U.build(curve, "x_zero")
    assert ok.device(MO, ctx)[0] == ok.oracle()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_f_at_infinity(MO, ctx_of, curve):
    """one polynomial at n points: f_0 = 0, so f = 0, and with f_blind = 0 its commitment is the identity"""
    import snark_verifier_amd as sv

    ctx = ctx_of(curve)
    c = U.build(curve, "m_eq_n_k1", n_polys=1, pairs=U.SHAPES["m_eq_n_k1"].pairs(curve)[:2], f_blind=0, tag="f-infinity")
    try:
        assert U.largest(c.sets) == (1, 1, 2) and c.n == 2
        with pytest.raises(U.T.TranscriptError, match=INFINITY_TEXT):
            c.oracle()
        _refused(MO, ctx, c, sv.SNARKV_ERR_ENCODING, [INFINITY_TEXT, "(f)"])
    finally:
        c.close()
    ok = U.build(curve, "m_eq_n_k1")
    assert ok.device(MO, ctx)[0] == ok.oracle()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_seeded_differential(MO, ctx_of, curve, k):
    ctx, ran = ctx_of(curve), 0
    for i, (n_polys, pairs) in enumerate(U.random_pair_lists(curve, k)):
        c = U.ShapeCase(curve, k, n_polys, pairs, "differential-%d" % i)
        try:
            proof, _ = c.device(MO, ctx)
            assert len(proof) == MO.proof_bytes(k, c.n_sets)
            assert proof == c.oracle(), (i, n_polys, pairs)
        finally:
            c.close()
        ran += 1
    assert ran == U.RANDOM_LISTS == 12
