"""GPU: the KZG multi-open provers (csrc/kzg_multiopen.hip) at the query shapes of tests/kzg_multiopen_util.py::SHAPES, each
there for a line of the provers, of their plan, of csrc/poly.hip or of csrc/msm_api.hip: sets of more than 32 polynomials, an L
of exactly 32 and 33 terms, 64 and 65 sets (one and two rounds of the MSM batch), divisions across the scan's block and level
boundaries, as many points as coefficients, a job of zero scalars, z = 0, a circuit's rotations.  Everything is byte for byte
against the Python prover of the util, which tests/test_kzg_multiopen_shapes.py pins with the oracle's verifiers.

  * both schemes, host and _dev forms, at every shape; the device's decide on what the oracle's verifier makes of the outputs
  * the _dev form between guards; shapes alternating on one context; a context whose first call is the prover
  * wrong evaluations: past term 31, at the third of five points, in two sets at once, in the second round of the batch
  * a repeated (polynomial, shift) with a wrong second evaluation: Gwc19 refuses, Bdfg21 uses the first
  * z' on a point of a set, z' = 0; the plan's refusals; SNARKV_FLAG_VALIDATE and SNARKV_FLAG_MONTGOMERY as context defaults
  * a seeded differential over random query lists"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import kzg_multiopen_util as U  # noqa: E402
from test_kzg_multiopen_shapes import repeat_case  # noqa: E402

pytestmark = pytest.mark.gpu
R = O.R
ZERO64 = b"\x00" * 64
MISMATCH = "evaluation does not match the polynomial (query set %d)"
DEV_GUARDED = ["np33", "S65", "m5_1000", "m3_65537", "m_eq_n_2"]  # the shapes the _dev form is run at on its own


@pytest.fixture(scope="module")
def KM():
    from snark_verifier_amd import kzg_multiopen

    return kzg_multiopen


@pytest.fixture(scope="module")
def sv():
    import snark_verifier_amd

    return snark_verifier_amd


@pytest.fixture(scope="module")
def dk_of(gpu_ctx, sv):
    """secret -> the deciding key with [secret] g2, made once each"""
    keys = {}

    def get(secret):
        if secret not in keys:
            keys[secret] = sv.DecidingKey(gpu_ctx, O.g1_to_bytes(O.G1_GEN), O.g2_to_bytes(O.G2_GEN),
                                          O.g2_to_bytes(O.g2_mul(O.G2_GEN, secret)))
        return keys[secret]

    yield get
    for key in keys.values():
        key.close()


@pytest.fixture(scope="module")
def resident(gpu_ctx):
    """name -> the catalogue entry resident between guards, evaluated by the device once; shared: leave it unchanged"""
    made = {}

    def get(name):
        if name not in made:
            c = U.build(name)
            made[name] = U.Resident(gpu_ctx, U.srs_of(c.secret, c.n), c.polys, c.z, c.pairs, guard=True)
            assert made[name].queries == c.queries  # the device's evaluations are Horner's
        return made[name]

    return get


@pytest.fixture(scope="module")
def plonk257(gpu_ctx):
    import random

    polys, z, queries = U.standard_plonk_instance(random.Random("gpu-kzg-shapes-plonk"), 257)
    return U.Resident(gpu_ctx, U.srs_of(U.SECRET, 257), polys, z, [(p, sh) for p, sh, _ in queries], guard=True)


def on_host(secret, res, queries, tag, draw=None):
    """the Python prover on the challenges of `tag` -> (ws, (w, z', w'))"""
    v, _, mu, gamma = U.challenges(tag)
    return (U.gwc19_prove(secret, res.polys, res.z, queries, v),
            U.bdfg21_prove(secret, res.polys, res.z, queries, mu, gamma, draw or U.draw_from(tag)))


def on_device(KM, ctx, res, queries, tag, form="dev", draw=None):
    """both provers through the module's wrappers, which raise on a refusal -> (ws, (w, z', w'))"""
    v, _, mu, gamma = U.challenges(tag)
    draw = draw or U.draw_from(tag)
    n_polys = len(res.polys)
    if form == "host":
        return (KM.gwc19_create_proof(ctx, res.srs, res.polys, res.z, queries, v),
                KM.bdfg21_create_proof(ctx, res.srs, res.polys, res.z, queries, mu, gamma, draw))
    return (KM.gwc19_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, n_polys, res.z, queries, v),
            KM.bdfg21_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, n_polys, res.z, queries, mu, gamma, draw))


def raw(KM, ctx, scheme, res, queries, tag, form="dev", draw=None, host_polys=None):
    """one raw C call on outputs filled with 0xA5 -> (code, message, the output buffers afterwards, the Ws the callback saw).
    `draw`: W bytes -> z' as an int or 32 bytes; `host_polys`: the packed polynomials of the host form, when not res.polys"""
    from snark_verifier_amd.ipa_multiopen import pack_queries

    a = KM.api()
    fe = lambda x: x if isinstance(x, bytes) else int(x).to_bytes(32, "little")  # noqa: E731
    v, _, mu, gamma = U.challenges(tag)
    draw = draw or U.draw_from(tag)
    qp, qs, qe, nq = pack_queries(queries)
    n_polys, seen = len(res.polys), []
    if form == "dev":
        head = (ctx._h, res.d_srs.data_ptr(), res.d_polys.data_ptr())
    else:
        head = (ctx._h, res.srs, host_polys if host_polys is not None else b"".join(U.pack(p) for p in res.polys))
    head += (res.n, n_polys, fe(res.z), qp, qs, qe, nq)
    if scheme == "gwc19":
        ws, count = ctypes.create_string_buffer(b"\xa5" * (64 * nq), 64 * nq), ctypes.c_size_t(0)
        fn = a.kzg_gwc19_create_proof_dev if form == "dev" else a.kzg_gwc19_create_proof
        rc = fn(*head, fe(v), ws, nq, ctypes.byref(count))
        return rc, a.last_error(), (ws.raw,), seen
    w, zp, wp = (ctypes.create_string_buffer(b"\xa5" * m, m) for m in (64, 32, 64))

    def cb(_user, w64, out32):
        seen.append(bytes(w64[:64]))
        ctypes.memmove(out32, fe(draw(seen[-1])), 32)
        return 0

    fn = a.kzg_bdfg21_create_proof_dev if form == "dev" else a.kzg_bdfg21_create_proof
    rc = fn(*head, fe(mu), fe(gamma), KM.CHALLENGE_FN(cb), None, w, zp, wp)
    return rc, a.last_error(), (w.raw, zp.raw, wp.raw), seen


def refused(KM, ctx, scheme, res, queries, tag, code, text, calls=0, **kw):
    rc, err, outs, seen = raw(KM, ctx, scheme, res, queries, tag, **kw)
    assert rc == code and text in err, (scheme, rc, err)
    assert all(o == b"\xa5" * len(o) for o in outs), scheme  # the outputs are written on success only
    assert len(seen) == calls, scheme


def with_eval(queries, changes):
    """the query list with {query index: what is added to its evaluation}"""
    out = list(queries)
    for at, d in changes.items():
        out[at] = (out[at][0], out[at][1], (out[at][2] + d) % R)
    return out


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.SHAPES))
def test_parity_at_every_shape(gpu_ctx, KM, dk_of, resident, name):
    c, sh, res = U.build(name), U.SHAPES[name], resident(name)
    assert U.claim_of(U.GWC19, res.queries) == sh.gwc19 and U.claim_of(U.BDFG21, res.queries) == sh.bdfg21
    assert KM.n_sets(KM.MOS_GWC19, res.queries) == sh.gwc19.n_sets and KM.n_sets(KM.MOS_BDFG21, res.queries) == sh.bdfg21.n_sets
    # the device decides what the oracle's verifier makes of a scheme's outputs unless one of them is the identity
    decide = ("gwc19", "bdfg21") if not c.identity else ("bdfg21",)
    ws, (w, _, wp) = U.check_case(gpu_ctx, KM, dk_of(c.secret), c.secret, res, name, decide=decide)
    assert [i for i, x in enumerate(ws) if x == ZERO64] == list(c.identity)
    assert w != ZERO64 and wp != ZERO64


@pytest.mark.parametrize("name", DEV_GUARDED)
def test_the_dev_form_between_guards(gpu_ctx, KM, resident, name):
    """the same bytes from an SRS and polynomials in device memory; both, and 4096 bytes on either side of each, unchanged"""
    c, res = U.build(name), resident(name)
    assert res.d_srs.data_ptr() % 16 == 0 and res.d_polys.data_ptr() % 16 == 0
    assert on_device(KM, gpu_ctx, res, res.queries, name) == on_host(c.secret, res, res.queries, name)
    assert res.unchanged()


def test_one_context_changing_shapes(gpu_ctx, KM, resident, plonk257):
    """plonk-257 (S = 3), S65 (two rounds, a new batch shape, 33 job contexts), np65, plonk-257 again: the schemes interleaved,
    every result the model's, the last bytes the first"""
    v, _, mu, gamma = U.challenges("alternate")
    draw = U.draw_from("alternate")
    got = []
    for name in ("plonk", "S65", "np65", "plonk"):
        res = plonk257 if name == "plonk" else resident(name)
        secret = U.SECRET if name == "plonk" else U.build(name).secret
        n_polys = len(res.polys)
        ws = KM.gwc19_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, res.n, n_polys, res.z, res.queries, v)
        bd = KM.bdfg21_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, res.n, n_polys, res.z, res.queries, mu, gamma, draw)
        ws2 = KM.gwc19_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, res.n, n_polys, res.z, res.queries, v)
        assert (ws, bd) == on_host(secret, res, res.queries, "alternate") and ws2 == ws, name
        got.append((ws, bd))
    assert got[3] == got[0] and len(got[0][0]) == 3 and len(got[1][0]) == 65


@pytest.mark.parametrize("scheme,name", [("gwc19", "S65"), ("bdfg21", "m5_1000")])
def test_the_first_call_on_a_fresh_context(sv, KM, resident, scheme, name):
    """the lanes, the job contexts and the high-priority streams are made inside the prover"""
    c, res = U.build(name), resident(name)  # evaluated on the shared context: the new one has seen no call
    v, _, mu, gamma = U.challenges(name)
    want_ws, want_bd = on_host(c.secret, res, res.queries, name)
    ctx = sv.Context(0)
    try:
        if scheme == "gwc19":
            assert KM.gwc19_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, len(res.polys), res.z, res.queries, v) == want_ws
        else:
            assert KM.bdfg21_create_proof_dev(ctx, res.d_srs, res.d_polys, res.n, len(res.polys), res.z, res.queries, mu, gamma,
                                              U.draw_from(name)) == want_bd
        assert on_device(KM, ctx, res, res.queries, name, form="host") == (want_ws, want_bd)
    finally:
        ctx.close()


# ---- wrong evaluations ----------------------------------------------------------------------------------------------------------
def _at(queries, poly, shift):
    at, = [i for i, q in enumerate(queries) if q[:2] == (poly, shift)]
    return at


def _wrong_cases():
    """name -> (shape, {query: delta}, the set Gwc19 names, the set Bdfg21 names)"""
    w = U.omega16()
    rot = U.SHAPES["rotations"].pairs()
    in1, in3 = _at(rot, 13, w), _at(rot, 17, w * w % R)
    m5 = U.SHAPES["m5_1000"].pairs()
    return {
        "term 33 of np65": ("np65", {32: 1}, 0, 0),
        "term 65 of np65": ("np65", {64: 5}, 0, 0),
        # Bdfg21: the third point of set 0; Gwc19: the set of that shift, its third
        "the third of five points": ("m5_1000", {_at(m5, 0, U.shift(2)): 1}, 2, 0),
        "the last of five points": ("m5_1000", {_at(m5, 0, U.shift(4)): R - 1}, 4, 0),
        "two bad sets": ("rotations", {in1: 1, in3: 1}, 1, 1),
        "the upper of the two alone": ("rotations", {in3: 1}, 3, 3),
        "three bad sets of S65": ("S65", {64: 1, 40: 1, 33: 2}, 33, 33),
        "set 64 of S65, in the second round": ("S65", {64: 1}, 64, 64),
    }


WRONG = _wrong_cases()


@pytest.mark.parametrize("case", list(WRONG))
def test_wrong_evaluations(gpu_ctx, sv, KM, resident, case):
    name, changes, set_g, set_b = WRONG[case]
    c, res = U.build(name), resident(name)
    bad = with_eval(res.queries, changes)
    v, _, mu, _ = U.challenges(case)
    # the model says which set leaves a remainder
    assert U.first_bad_set(U.GWC19, res.polys, res.z, bad, v) == set_g and U.first_bad_set(U.BDFG21, res.polys, res.z, bad, mu) == set_b
    refused(KM, gpu_ctx, "gwc19", res, bad, case, sv.SNARKV_ERR_ARG, MISMATCH % set_g)
    refused(KM, gpu_ctx, "bdfg21", res, bad, case, sv.SNARKV_ERR_ARG, MISMATCH % set_b)  # draw_z_prime is not called
    refused(KM, gpu_ctx, "gwc19", res, bad, case, sv.SNARKV_ERR_ARG, MISMATCH % set_g, form="host")
    assert on_device(KM, gpu_ctx, res, res.queries, case) == on_host(c.secret, res, res.queries, case)  # the context opens on


def test_a_repeated_query_with_a_wrong_second_evaluation(gpu_ctx, sv, KM):
    """Gwc19 keeps both evaluations and refuses; Bdfg21 keeps the first and gives the bytes of the list without the repeat"""
    polys, z, given, clean = repeat_case()
    res = U.Resident(gpu_ctx, U.srs_of(U.SECRET, 9), polys, z, [q[:2] for q in given])
    assert res.queries[:4] == clean and res.queries[4] == clean[2]  # the device's evaluations: the repeat's is the first's
    v, _, mu, _ = U.challenges("repeat")
    # the model first: Gwc19's set 1 leaves a remainder, no set of Bdfg21 does
    assert U.first_bad_set(U.GWC19, polys, z, given, v) == 1 and U.first_bad_set(U.BDFG21, polys, z, given, mu) is None
    want_ws, want_bd = on_host(U.SECRET, res, clean, "repeat")
    assert on_host(U.SECRET, res, given, "repeat")[1] == want_bd
    for form in ("dev", "host"):
        refused(KM, gpu_ctx, "gwc19", res, given, "repeat", sv.SNARKV_ERR_ARG, MISMATCH % 1, form=form)
        rc, _, outs, seen = raw(KM, gpu_ctx, "bdfg21", res, given, "repeat", form=form)
        assert rc == 0 and (outs[0], int.from_bytes(outs[1], "little"), outs[2]) == want_bd and seen == [want_bd[0]]
    assert on_device(KM, gpu_ctx, res, clean, "repeat") == (want_ws, want_bd)
    # the repeat with the right evaluation is two terms of Gwc19's set, and fine
    assert on_device(KM, gpu_ctx, res, res.queries, "repeat") == on_host(U.SECRET, res, res.queries, "repeat")


# ---- z' -----------------------------------------------------------------------------------------------------------------------
def test_z_prime_on_a_point_of_a_set(gpu_ctx, sv, KM, resident):
    c, res = U.build("rotations"), resident("rotations")
    sets = U.sets_of(U.BDFG21, res.queries)
    w = sets[1]["shifts"][1]
    assert w not in sets[0]["shifts"] and w in sets[3]["shifts"]  # set 1 is the first that has the point z w
    for form in ("dev", "host"):
        refused(KM, gpu_ctx, "bdfg21", res, res.queries, "zp", sv.SNARKV_ERR_ARG, "z' is a point of query set 1", calls=1,
                draw=lambda _w: c.z * w % R, form=form)
    refused(KM, gpu_ctx, "bdfg21", res, res.queries, "zp", sv.SNARKV_ERR_ARG, "z' is a point of query set 3", calls=1,
            draw=lambda _w: c.z * sets[3]["shifts"][3] % R)
    assert on_device(KM, gpu_ctx, res, res.queries, "zp") == on_host(c.secret, res, res.queries, "zp")
    # z' = 0 is legal
    zero = lambda _w: 0  # noqa: E731
    got = on_device(KM, gpu_ctx, res, res.queries, "zp", draw=zero)
    assert got == on_host(c.secret, res, res.queries, "zp", draw=zero) and got[1][1] == 0


# ---- the plan's refusals ------------------------------------------------------------------------------------------------------
def test_z_zero_with_a_two_shift_set(gpu_ctx, sv, KM, resident):
    c = U.build("z_zero")
    res = U.Resident(gpu_ctx, U.srs_of(c.secret, c.n), c.polys, 0, c.pairs + [(2, U.shift(1))])
    assert U.plan_status(U.BDFG21, res.queries, c.n, 0) == (U.PLAN_COINCIDE, 2)  # polynomial 2 now has two shifts, and one point
    for form in ("dev", "host"):
        refused(KM, gpu_ctx, "bdfg21", res, res.queries, "z0", sv.SNARKV_ERR_ARG, "two points of query set 2 coincide", form=form)
    v = U.challenges("z0")[0]
    ws = KM.gwc19_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, res.n, 3, 0, res.queries, v)
    assert ws == U.gwc19_prove(c.secret, c.polys, 0, res.queries, v) and len(ws) == 3  # Gwc19's sets have one point each
    ok = resident("z_zero")
    assert on_device(KM, gpu_ctx, ok, ok.queries, "z0") == on_host(c.secret, ok, ok.queries, "z0")


@pytest.mark.parametrize("n", [1, 2])
def test_more_points_than_coefficients(gpu_ctx, sv, KM, n):
    import random

    rng = random.Random("kzg-n-plus-one-%d" % n)
    polys, z = [[rng.randrange(R) for _ in range(n)] for _ in range(2)], rng.randrange(1, R)
    res = U.Resident(gpu_ctx, U.srs_of(U.SECRET, n), polys, z, [(0, 1)] + [(1, U.shift(j)) for j in range(n + 1)])
    assert U.plan_status(U.BDFG21, res.queries, n, z) == (U.PLAN_TOO_MANY_POINTS, 1)
    for form in ("dev", "host"):
        refused(KM, gpu_ctx, "bdfg21", res, res.queries, "n+1", sv.SNARKV_ERR_ARG, "query set 1 has more points than", form=form)
    # n points are allowed on the same context, and Gwc19 takes the n + 1 shifts as n + 1 sets
    fewer = res.queries[:-1]
    assert on_device(KM, gpu_ctx, res, fewer, "n+1") == on_host(U.SECRET, res, fewer, "n+1")
    v = U.challenges("n+1")[0]
    assert KM.gwc19_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, n, 2, z, res.queries, v) == U.gwc19_prove(U.SECRET, polys, z, res.queries, v)


# ---- the context's default flags ------------------------------------------------------------------------------------------------
def test_validate_as_the_context_default(gpu_ctx, sv, KM, resident):
    c, res = U.build("L33"), resident("L33")
    want = on_host(c.secret, res, res.queries, "validate")
    # a polynomial whose last coefficient is zero, spelt r: the value is the same, the bytes are not canonical
    polys = [list(p) for p in c.polys]
    polys[-1][-1] = 0
    spelt = b"".join(U.pack(p) for p in polys[:-1]) + U.pack(polys[-1][:-1]) + R.to_bytes(32, "little")
    alias = U.Resident(gpu_ctx, U.srs_of(c.secret, c.n), polys, c.z, c.pairs)
    d_spelt = U.to_dev(spelt)
    sh = res.queries[-1][1]
    assert sh != 1 and sh + R < 1 << 256 and res.queries[-1][2] + R < 1 << 256
    two_encodings = res.queries + [(res.queries[-1][0], sh + R, res.queries[-1][2])]
    assert gpu_ctx.get_flags() == 0
    gpu_ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
    try:
        for form in ("dev", "host"):
            assert on_device(KM, gpu_ctx, res, res.queries, "validate", form=form) == want  # clean inputs: the same bytes
        for scheme in ("gwc19", "bdfg21"):
            # a coefficient: counted on the device, in both forms
            alias.d_polys = d_spelt
            refused(KM, gpu_ctx, scheme, alias, alias.queries, "validate", sv.SNARKV_ERR_ENCODING, "1 coefficients")
            refused(KM, gpu_ctx, scheme, alias, alias.queries, "validate", sv.SNARKV_ERR_ENCODING, "1 coefficients", form="host",
                    host_polys=spelt)
            # a shift, an evaluation: on the host
            for bad in (res.queries[:-1] + [(res.queries[-1][0], sh + R, res.queries[-1][2])],
                        res.queries[:-1] + [(res.queries[-1][0], sh, res.queries[-1][2] + R)], two_encodings):
                refused(KM, gpu_ctx, scheme, res, bad, "validate", sv.SNARKV_ERR_ENCODING, "not canonical")
        # z' from the callback, after W
        big = lambda w: (U.draw_from("validate")(w) % ((1 << 256) - R)) + R  # noqa: E731
        refused(KM, gpu_ctx, "bdfg21", res, res.queries, "validate", sv.SNARKV_ERR_ENCODING, "z' is not canonical", calls=1, draw=big)
        assert on_device(KM, gpu_ctx, res, res.queries, "validate") == want
    finally:
        gpu_ctx.set_flags(0)
    # without the flag two encodings of one shift are two shifts of one point: Bdfg21's coincide refusal, two sets with equal W
    # for Gwc19
    status, bad_set = U.plan_status(U.BDFG21, two_encodings, c.n, c.z)
    assert status == U.PLAN_COINCIDE
    refused(KM, gpu_ctx, "bdfg21", res, two_encodings, "validate", sv.SNARKV_ERR_ARG, "two points of query set %d coincide" % bad_set)
    polys, z, _, clean = repeat_case()
    w = clean[2][1]
    pair = U.Resident(gpu_ctx, U.srs_of(U.SECRET, 9), polys, z, [(0, 1), (1, w), (1, w + R)])
    assert U.plan_status(U.BDFG21, pair.queries, 9, z) == (U.PLAN_COINCIDE, 1) and pair.queries[1][2] == pair.queries[2][2]
    refused(KM, gpu_ctx, "bdfg21", pair, pair.queries, "validate", sv.SNARKV_ERR_ARG, "two points of query set 1 coincide")
    v = U.challenges("validate")[0]
    ws = KM.gwc19_create_proof_dev(gpu_ctx, pair.d_srs, pair.d_polys, 9, 3, z, pair.queries, v)
    assert ws == U.gwc19_prove(U.SECRET, polys, z, pair.queries, v) and len(ws) == 3 and ws[1] == ws[2] != ws[0]
    gpu_ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
    try:
        refused(KM, gpu_ctx, "gwc19", pair, pair.queries, "validate", sv.SNARKV_ERR_ENCODING, "not canonical")
    finally:
        gpu_ctx.set_flags(0)


def test_montgomery_as_the_context_default(gpu_ctx, sv, KM, resident):
    """the KZG calls speak the wire form whatever the default says (include/snarkv_kzg_multiopen.h), and leave the default"""
    import coracle as C
    import mont_util as M

    s, p = C.sample_scalars(0x4B5A, 40), C.sample_points(0x4B5B, 40)
    canonical = gpu_ctx.msm_pippenger(s, p)
    assert canonical == C.msm_pippenger(s, p, 2)
    ctx = sv.Context(0)
    try:
        ctx.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
        for name in ("S65", "rotations"):  # the batch's job contexts take the call's encoding, not the default
            c, res = U.build(name), resident(name)
            want = on_host(c.secret, res, res.queries, "mont")
            for form in ("dev", "host"):
                assert on_device(KM, ctx, res, res.queries, "mont", form=form) == want, (name, form)
                assert ctx.get_flags() == sv.SNARKV_FLAG_MONTGOMERY
                got = ctx.msm_pippenger(M.scalars_to_mont(s), M.coords_to_mont(p))  # the default is still in force
                assert M.coords_from_mont(got) == canonical and got != canonical, (name, form)
            assert on_device(KM, gpu_ctx, res, res.queries, "mont") == want  # the flag-free context
    finally:
        ctx.close()


# ---- the seeded differential ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", U.RANDOM_NS)
def test_seeded_differential(gpu_ctx, sv, KM, n):
    ran = refusals = 0
    for i, (polys, z, queries) in enumerate(U.random_query_lists(n)):
        tag = "differential %d %d" % (n, i)
        res = U.Resident(gpu_ctx, U.srs_of(U.SECRET, n), polys, z, [q[:2] for q in queries])
        assert res.queries == queries
        status, bad_set = U.plan_status(U.BDFG21, queries, n, z)
        if status != U.PLAN_OK:  # refused by the plan: refused by the device with the same set, not skipped
            text = {U.PLAN_TOO_MANY_POINTS: "query set %d has more points than", U.PLAN_COINCIDE: "two points of query set %d coincide"}
            for form in ("dev", "host"):
                refused(KM, gpu_ctx, "bdfg21", res, queries, tag, sv.SNARKV_ERR_ARG, text[status] % bad_set, form=form)
            v = U.challenges(tag)[0]
            assert KM.gwc19_create_proof_dev(gpu_ctx, res.d_srs, res.d_polys, n, len(polys), z, queries, v) == \
                U.gwc19_prove(U.SECRET, polys, z, queries, v)
            refusals += 1
        else:
            want = on_host(U.SECRET, res, queries, tag)
            for form in ("dev", "host"):
                assert on_device(KM, gpu_ctx, res, queries, tag, form=form) == want, (n, i, form)
        ran += 1
    assert ran == U.RANDOM_LISTS == 12 and 4 * refusals <= ran
