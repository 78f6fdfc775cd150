"""GPU: the KZG multi-open provers on BN254 (snark_verifier_amd.kzg_multiopen, include/snarkv_kzg_multiopen.h), in the flow
polynomials -> evaluations -> opening: the SRS comes from a toy secret, the polynomials are resident, and the evaluations the
provers are handed come from `poly_batch.eval_many_dev` on those resident polynomials.

  1  17 polynomials in the shape of oracle/kzg.py::standard_plonk_queries at n = 4, 257, 1000 (one block of the scan, two,
     four and no power of two), both schemes, host and _dev forms: the bytes are those of the Python prover
     (tests/kzg_multiopen_util.py, pinned by the oracle's verifiers in tests/test_kzg_multiopen_model.py), the oracle's
     verifier gives lhs == [s] rhs on them, and snarkv_kzg_decide accepts lhs || rhs under the key with [s] g2
  2  set shapes: one polynomial with one query; 40 polynomials in one set (two passes of the linear combination); a
     (polynomial, shift) pair given twice; three points at n = 3 next to a second set and alone (W is the identity); constants
     (every output the identity)
  3  one wrong evaluation, per scheme: SNARKV_ERR_ARG naming the set, the outputs untouched, the context usable afterwards;
     the same for a callback that fails
  4  the C++ mirror (`Gwc19::create_proof` / `Bdfg21::create_proof`, host/pcs.hpp) through its test hook, over the EVM and the
     Poseidon transcript with a non-empty prefix: `read` + `pcs_verify` + decide accept; with one byte flipped they do not;
     the product call (snark_verifier_amd.host_kzg_open) writes the mirror's bytes"""
import ctypes
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

pytestmark = pytest.mark.gpu
R = O.R
SECRET = 0x7A11_5EC2_E7
ZERO64 = b"\x00" * 64
ERR_ARG = -5


@pytest.fixture(scope="module")
def KM():
    from snark_verifier_amd import kzg_multiopen

    return kzg_multiopen


@pytest.fixture(scope="module")
def srs_bytes():
    """[s^i] G for i < 1000, once; a shorter SRS is its head"""
    return U.srs_of(SECRET, 1000)


@pytest.fixture(scope="module")
def dk(gpu_ctx):
    import snark_verifier_amd as sv

    key = sv.DecidingKey(gpu_ctx, O.g1_to_bytes(O.G1_GEN), O.g2_to_bytes(O.G2_GEN), O.g2_to_bytes(O.g2_mul(O.G2_GEN, SECRET)))
    yield key
    key.close()


Resident = U.Resident  # the device flow is shared with tests/test_gpu_kzg_multiopen_shapes.py


def check_case(gpu_ctx, KM, dk, res, tag, **kw):
    return U.check_case(gpu_ctx, KM, dk, SECRET, res, tag, **kw)


@pytest.mark.parametrize("n", [4, 257, 1000])
def test_standard_plonk_shape(gpu_ctx, KM, dk, srs_bytes, n):
    rng = random.Random("gpu-kzg-plonk-%d" % n)
    polys, z, queries = U.standard_plonk_instance(rng, n)
    res = Resident(gpu_ctx, srs_bytes, polys, z, [(p, sh) for p, sh, _ in queries])
    assert KM.n_sets(KM.MOS_GWC19, res.queries) == 3 and KM.n_sets(KM.MOS_BDFG21, res.queries) == 4
    check_case(gpu_ctx, KM, dk, res, "plonk %d" % n)


SHAPES = U.set_shape_cases(random.Random("gpu-kzg-set-shapes"))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_set_shapes(gpu_ctx, KM, dk, srs_bytes, name):
    polys, z, queries = SHAPES[name]
    res = Resident(gpu_ctx, srs_bytes, polys, z, [(p, sh) for p, sh, _ in queries])
    identity = name in ("three points at n = 3, alone", "constants, n = 1")
    ws, (w, _, wp) = check_case(gpu_ctx, KM, dk, res, name, decide=not identity)
    if name == "three points at n = 3, alone":
        assert w == ZERO64 and wp != ZERO64  # h = 0; L = q - q(z') is not
    if name == "constants, n = 1":
        assert ws == [ZERO64] * 2 and w == wp == ZERO64
    if name == "40 polynomials in one set":
        from snark_verifier_amd import poly

        assert len(polys) > poly.LINCOMB_TERMS


def test_one_wrong_evaluation_is_refused_and_the_context_stays_usable(gpu_ctx, KM, srs_bytes):
    rng = random.Random("gpu-kzg-wrong")
    polys, z, queries = U.standard_plonk_instance(rng, 257)
    res = Resident(gpu_ctx, srs_bytes, polys, z, [(p, sh) for p, sh, _ in queries])
    a = KM.api()
    v, mu, gamma = (rng.randrange(1, R) for _ in range(3))
    fe = lambda x: int(x).to_bytes(32, "little")  # noqa: E731
    called = []

    def run(queries, draw_rc=0):
        """the raw calls on pattern-filled outputs -> (rc gwc19, rc bdfg21, the output buffers)"""
        from snark_verifier_amd.ipa_multiopen import pack_queries

        qp, qs, qe, nq = pack_queries(queries)
        ws, count = ctypes.create_string_buffer(b"\xa5" * (64 * nq), 64 * nq), ctypes.c_size_t(0)
        w, zp, wp = (ctypes.create_string_buffer(b"\xa5" * 64, 64) for _ in range(3))

        def cb(_user, w64, out32):
            called.append(bytes(w64[:64]))
            ctypes.memmove(out32, fe(U.draw_from("wrong")(bytes(w64[:64]))), 32)
            return draw_rc

        head = (gpu_ctx._h, res.d_srs.data_ptr(), res.d_polys.data_ptr(), res.n, len(polys), fe(z), qp, qs, qe, nq)
        rc_g = a.kzg_gwc19_create_proof_dev(*head, fe(v), ws, nq, ctypes.byref(count))
        err_g = a.last_error()
        rc_b = a.kzg_bdfg21_create_proof_dev(*head, fe(mu), fe(gamma), KM.CHALLENGE_FN(cb), None, w, zp, wp)
        return rc_g, err_g, rc_b, a.last_error(), (ws.raw, w.raw, zp.raw, wp.raw)

    untouched = (b"\xa5" * (64 * len(queries)), b"\xa5" * 64, b"\xa5" * 64, b"\xa5" * 64)
    # query 19 is polynomial 11 at the second shift: Gwc19's set 1 (by shift), and Bdfg21's set 1 ({1, w}: polynomials 3, 11)
    assert res.queries[19][0] == 11 and [st["polys"] for st in K.bdfg21_query_sets(res.queries)][1] == [3, 11]
    bad = list(res.queries)
    bad[19] = (bad[19][0], bad[19][1], (bad[19][2] + 1) % R)
    rc_g, err_g, rc_b, err_b, outs = run(bad)
    assert rc_g == ERR_ARG and "evaluation does not match the polynomial (query set 1)" in err_g
    assert rc_b == ERR_ARG and "evaluation does not match the polynomial (query set 1)" in err_b
    assert outs == untouched and called == []  # refused at the first synchronisation: the transcript never saw W
    # a callback that fails: SNARKV_ERR_ARG after it ran once, nothing written
    rc_g, _, rc_b, err_b, outs = run(res.queries, draw_rc=1)
    assert rc_g == 0 and rc_b == ERR_ARG and "draw_z_prime" in err_b and len(called) == 1
    assert outs[1:] == untouched[1:]
    # ... and the same context opens correctly afterwards
    rc_g, _, rc_b, _, outs = run(res.queries)
    assert rc_g == 0 and rc_b == 0 and len(called) == 2
    want_ws = U.gwc19_prove(SECRET, polys, z, res.queries, v)
    want = U.bdfg21_prove(SECRET, polys, z, res.queries, mu, gamma, U.draw_from("wrong"))
    assert outs[0][:64 * 3] == b"".join(want_ws) and outs[0][64 * 3:] == untouched[0][64 * 3:]
    assert (outs[1], int.from_bytes(outs[2][:32], "little"), outs[3]) == want and outs[2][32:] == b"\xa5" * 32


@pytest.fixture(scope="module")
def hook():
    import importlib.util

    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build_host_driver()
    lib = ctypes.CDLL(b.HOSTTEST_LIB)
    vp, cp, sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
    lib.hd_kzg_open_roundtrip.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, sz, sz, cp, cp, vp, cp, cp, sz, cp, sz, cp, sz, vp, sz,
                                          ctypes.POINTER(sz)]
    return lib


@pytest.mark.parametrize("tkind", [0, 1], ids=["evm", "poseidon"])
@pytest.mark.parametrize("mos", [0, 1], ids=["gwc19", "bdfg21"])
def test_mirror_round_trip(gpu_ctx, srs_bytes, hook, mos, tkind):
    from snark_verifier_amd.ipa_multiopen import pack_queries

    rng = random.Random("gpu-kzg-mirror")
    n = 257
    polys, z, queries = U.standard_plonk_instance(rng, n)
    res = Resident(gpu_ctx, srs_bytes, polys, z, [(p, sh) for p, sh, _ in queries])
    cms = b"".join(U.mulg(U.horner(p, SECRET)) for p in polys)
    # the prefix: two commitments, a squeeze, a scalar, another squeeze -- a transcript in the middle of a proof
    prefix = b"\x01" + cms[:64] + b"\x01" + cms[64:128] + b"\x02" + b"\x00" + (12345).to_bytes(32, "little") + b"\x02"
    prefix_bytes = 64 * 2 + 32 if tkind == 0 else 32 * 2 + 32  # the Poseidon transcript writes compressed points
    dk320 = O.g1_to_bytes(O.G1_GEN) + O.g2_to_bytes(O.G2_GEN) + O.g2_to_bytes(O.g2_mul(O.G2_GEN, SECRET))
    qp, qs, qe, nq = pack_queries(res.queries)
    proof, plen = ctypes.create_string_buffer(4096), ctypes.c_size_t(0)

    def run(flip_at):
        return hook.hd_kzg_open_roundtrip(mos, tkind, gpu_ctx._h, res.d_srs.data_ptr(), res.d_polys.data_ptr(), n, len(polys), cms,
                                          z.to_bytes(32, "little"), qp, qs, qe, nq, prefix, len(prefix), dk320, flip_at, proof, 4096,
                                          ctypes.byref(plen))

    assert run(1 << 40) == 1
    point = 64 if tkind == 0 else 32
    assert plen.value == prefix_bytes + point * (3 if mos == 0 else 2)
    first = proof.raw[:plen.value]
    assert run(prefix_bytes + 5) != 1 and proof.raw[:plen.value] == first  # one byte of the first opening point flipped
    assert run(plen.value - 3) != 1                                         # ... of the last
    assert run(1 << 40) == 1
    # the product call on the same inputs: the bytes the opening wrote are the mirror's after the prefix
    from snark_verifier_amd import host_kzg_open as HK

    items = [("point", cms[:64]), ("point", cms[64:128]), ("squeeze",), ("scalar", 12345), ("squeeze",)]
    assert HK.pack_prefix(items) == prefix
    rc, written, challenges = HK.kzg_open(mos, tkind, gpu_ctx, res.d_srs, res.d_polys, n, len(polys), z, res.queries, items)
    assert rc == 1 and written == first[prefix_bytes:] and len(challenges) == (1 if mos == 0 else 3)
    bad = list(res.queries)
    bad[0] = (bad[0][0], bad[0][1], (bad[0][2] + 1) % R)
    rc, written, _ = HK.kzg_open(mos, tkind, gpu_ctx, res.d_srs, res.d_polys, n, len(polys), z, bad, items)
    assert rc == 0 and written == b""  # the mirror's assertion failure: the evaluation does not match
