"""GPU: the product C API of the pasta flavour of the host mirror (include/snarkv_host_pallas.h, libsnarkv_host_pallas.so,
snark_verifier_amd.host_api_pallas) against the oracle, on N = 33 PLONK-over-IPA proofs forged at k = 6 the way
tests/test_pallas_host_mirror.py forges them: batch succinct verification under the three decompression routes,
`plonk_verify`, the error cases, `decide_all`, the accumulation scheme (prover and verifier) and `aggregate`."""
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as BN  # noqa: E402
import ipa as I  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402
from ipa_util import pack_acc  # noqa: E402

pytestmark = pytest.mark.gpu
K, N = 6, 33


@pytest.fixture(scope="module")
def HPA():
    """the product library, built through build.py as the `HP` fixture of test_pallas_host_mirror.py builds the hooks"""
    import importlib.util

    from snark_verifier_amd import host_api_pallas as H
    from snark_verifier_amd import pallas as PL

    PL.load_library()
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build_host_api_pallas()
    H.load_library()
    return H


@pytest.fixture(scope="module")
def batch(HPA):
    import hostfmt
    import plonk as P
    import plonk_synth as S

    S.use_curve(PA)
    hostfmt.use_curve(PA)
    try:
        rng = random.Random("host-pallas-api")
        pr, dl = S.standard_plonk_protocol(rng, k=K, num_instance=(3,))
        kd = {"g": [rng.randrange(1, PA.R) for _ in range(1 << K)], "h": rng.randrange(1, PA.R), "s": rng.randrange(1, PA.R)}
        g = [PA.g1_mul(PA.G1_GEN, c) for c in kd["g"]]
        h, s = PA.g1_mul(PA.G1_GEN, kd["h"]), PA.g1_mul(PA.G1_GEN, kd["s"])
        mk = lambda stream=b"": T.Blake2bTranscript(PA, stream)  # noqa: E731
        insts = [[[rng.randrange(PA.R) for _ in range(3)]] for _ in range(N)]
        proofs = [P.forge_proof_ipa(pr, insts[i], kd, mk, rng, dl) for i in range(N)]
        accs = [P.succinct_verify_ipa(g[0], h, s, pr, insts[i], P.plonk_proof_read(pr, insts[i], mk(proofs[i]), "bgh19"))[0]
                for i in range(N)]
        b = {"pr": pr, "g": g, "h": h, "s": s, "insts": insts, "proofs": proofs, "accs": accs,
             "pbytes": S.pack_protocol(pr), "protocol": HPA.Protocol(S.pack_protocol(pr)),
             "ib": b"".join(S.pack_instances(x) for x in insts), "pb": HPA.pack_proofs(proofs),
             "pack_instances": S.pack_instances}
        gb = b"".join(PA.g1_to_bytes(p) for p in g)
        b["dk"] = HPA.IpaDecidingKey(K, gb, PA.g1_to_bytes(h), PA.g1_to_bytes(s))
        b["dk_nozk"] = HPA.IpaDecidingKey(K, gb, PA.g1_to_bytes(h))
        b["want"] = b"".join(pack_acc(a) for a in accs)
        yield b
        for key in ("dk", "dk_nozk", "protocol"):
            b[key].close()
    finally:
        S.use_curve(BN)
        hostfmt.use_curve(BN)


@pytest.fixture(scope="module")
def hooks(HPA):
    """the test-hook library: the layout pass and the batch reader with its count of hints taken"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = ctypes.CDLL(b.build_host_driver_pallas())
    h.hp_plonk_ipa_point_offsets.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    h.hp_plonk_ipa_read_batch.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                          ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_size_t)]
    return h


def _point_offsets(hooks, batch):
    """where the compressed points of a proof of the batch's protocol sit, from the layout pass itself"""
    offs, ln = (ctypes.c_uint32 * 64)(), ctypes.c_size_t(0)
    n = hooks.hp_plonk_ipa_point_offsets(batch["pbytes"], len(batch["pbytes"]), K, offs, 64, ctypes.byref(ln))
    assert n == 12 + 2 * K and ln.value == len(batch["proofs"][0])
    return list(offs[:n])


def _hints_taken(hooks, batch, pb, route, threads=4):
    import struct

    svk = struct.pack("<II", K, 1) + b"".join(PA.g1_to_bytes(p) for p in (batch["g"][0], batch["h"], batch["s"]))
    taken = ctypes.c_size_t(1 << 40)
    rc = hooks.hp_plonk_ipa_read_batch(batch["pbytes"], len(batch["pbytes"]), batch["ib"], len(batch["ib"]), pb, len(pb), N, svk,
                                       threads, route, ctypes.byref(taken))
    return rc, taken.value


@pytest.fixture()
def on_pallas():
    I.use_curve(PA)
    yield
    I.use_curve(BN)


def _routes(H):
    return (H.DECOMPRESS_HOST, H.DECOMPRESS_DEVICE, H.DECOMPRESS_AUTO)


def _raw_verify(H, b, ib, pb, n, route, threads=4):
    """the return code itself (the Python wrappers raise on negative codes)"""
    out = ctypes.create_string_buffer(b["dk"].acc_bytes * n)
    rc = H.load_library().snarkv_host_pallas_plonk_succinct_verify_batch(b["protocol"]._h, b["dk"]._h, ib, len(ib), pb, len(pb), n,
                                                                        threads, route, out, len(out))
    rc2 = H.load_library().snarkv_host_pallas_plonk_verify(b["protocol"]._h, b["dk"]._h, ib, len(ib), pb, len(pb), n, threads, route)
    return rc, rc2, out.raw


def test_succinct_verify_batch_three_routes_equal_the_oracle(HPA, batch):
    for route in _routes(HPA):
        for threads in (1, 4, 0):
            rc, accs = HPA.plonk_succinct_verify_batch(batch["protocol"], batch["dk"], batch["ib"], batch["pb"], N, threads, route)
            assert rc == 1 and accs == batch["want"], (route, threads)
        assert HPA.plonk_verify(batch["protocol"], batch["dk"], batch["ib"], batch["pb"], N, 4, route)
    # a smaller batch, and a buffer that is too small
    rc, accs = HPA.plonk_succinct_verify_batch(batch["protocol"], batch["dk"], batch["pack_instances"](batch["insts"][0]),
                                               HPA.pack_proofs(batch["proofs"][:1]), 1, 0, HPA.DECOMPRESS_DEVICE)
    assert rc == 1 and accs == batch["want"][:batch["dk"].acc_bytes]
    small = ctypes.create_string_buffer(batch["dk"].acc_bytes * N - 1)
    assert HPA.load_library().snarkv_host_pallas_plonk_succinct_verify_batch(
        batch["protocol"]._h, batch["dk"]._h, batch["ib"], len(batch["ib"]), batch["pb"], len(batch["pb"]), N, 0,
        HPA.DECOMPRESS_AUTO, small, len(small)) == HPA.ERR_CAPACITY


def test_device_route_reads_every_point_from_the_devices_answers(HPA, batch, hooks):
    """HOST and DEVICE give the same bytes by design, so equal accumulators cannot tell whether a transcript took a
    single hint: the reader counts them.  A clean batch under DEVICE takes all N x (12 + 2k); HOST none; a proof with a
    point the device refuses takes the hints in front of that point and fails there, on the host's square root."""
    import pallas_decompress_util as U

    per_proof = 12 + 2 * K
    assert _hints_taken(hooks, batch, batch["pb"], HPA.DECOMPRESS_HOST) == (1, 0)
    for threads in (1, 4):
        assert _hints_taken(hooks, batch, batch["pb"], HPA.DECOMPRESS_DEVICE, threads) == (1, N * per_proof)
    want_auto = N * per_proof if N >= HPA.DEVICE_MIN else 0
    assert _hints_taken(hooks, batch, batch["pb"], HPA.DECOMPRESS_AUTO) == (1, want_auto)
    offs = _point_offsets(hooks, batch)
    x_ns = next(x for x, _ in U.seeded_pairs(9, 50) if U.order_exponent((x * x * x + 5) % PA.P) == 32)
    j, q = 17, per_proof - 3  # one of Bgh19's L_i / R_i
    bad = bytearray(batch["proofs"][j])
    bad[offs[q]:offs[q] + 32] = U.encode(x_ns, 1)
    ps = list(batch["proofs"])
    ps[j] = bytes(bad)
    assert _hints_taken(hooks, batch, HPA.pack_proofs(ps), HPA.DECOMPRESS_DEVICE) == (-10, (N - 1) * per_proof + q)
    # a proof of another length is read without hints, the others with them
    ps[j] = batch["proofs"][j] + b"\x00"
    assert _hints_taken(hooks, batch, HPA.pack_proofs(ps), HPA.DECOMPRESS_DEVICE) == (1, (N - 1) * per_proof)


def test_error_cases_answer_alike_under_every_route(HPA, batch, hooks):
    import pallas_decompress_util as U

    j = 17
    layout_points = _point_offsets(hooks, batch)  # witnesses, quotient chunks, f, S, L_i / R_i, G
    assert layout_points[:9] == [32 * i for i in range(9)] and layout_points[9] > 32 * 9  # the evaluations lie between
    x_ns = next(x for x, _ in U.seeded_pairs(9, 50) if U.order_exponent((x * x * x + 5) % PA.P) == 32)

    def with_proof(j, proof):
        ps = list(batch["proofs"])
        ps[j] = bytes(proof)
        return HPA.pack_proofs(ps)

    cases = {}
    for pos in (0, 40, 300, len(batch["proofs"][j]) - 1):
        bad = bytearray(batch["proofs"][j])
        bad[pos] ^= 1
        cases["flip@%d" % pos] = (batch["ib"], with_proof(j, bad), None)
    insts = [[list(c) for c in x] for x in batch["insts"]]
    insts[j][0][1] = (insts[j][0][1] + 1) % PA.R
    cases["instance"] = (b"".join(batch["pack_instances"](x) for x in insts), batch["pb"], 0)
    last = len(layout_points) - 1
    for q in (0, 5, 9, 10, 11, last - 1, last):  # a witness, a quotient chunk, f, S, L_0, R_(k-1), G
        for par in (0, 1):
            bad = bytearray(batch["proofs"][j])
            bad[layout_points[q]:layout_points[q] + 32] = U.encode(x_ns, par)
            cases["non-residue@%d/%d" % (q, par)] = (batch["ib"], with_proof(j, bad), HPA.ERR_TRANSCRIPT)
    bad = bytearray(batch["proofs"][j])
    bad[layout_points[3]:layout_points[3] + 32] = U.encode(PA.P + 1, 0)  # x >= p
    cases["x>=p"] = (batch["ib"], with_proof(j, bad), HPA.ERR_TRANSCRIPT)
    bad[layout_points[3]:layout_points[3] + 32] = bytes(32)  # the identity's encoding
    cases["identity"] = (batch["ib"], with_proof(j, bad), HPA.ERR_TRANSCRIPT)
    cases["short"] = (batch["ib"], with_proof(j, batch["proofs"][j][:-1]), HPA.ERR_TRANSCRIPT)
    for name, (ib, pb, want) in cases.items():
        got = {route: _raw_verify(HPA, batch, ib, pb, N, route)[:2] for route in _routes(HPA)}
        host = got[HPA.DECOMPRESS_HOST]
        print(name, got)
        assert host[0] == host[1] and host[0] in (0, HPA.ERR_TRANSCRIPT), name
        assert all(v == host for v in got.values()), (name, got)
        if want is not None:
            assert host[0] == want, (name, host)


def test_decide_all_flags_exactly_the_planted_accumulator(HPA, batch):
    ok, each = HPA.ipa_decide_all(batch["dk"], batch["want"])
    assert ok and each == [True] * N
    accs = list(batch["accs"])
    accs[20] = (accs[20][0], PA.g1_add(accs[20][1], batch["h"]))
    ok, each = HPA.ipa_decide_all(batch["dk"], b"".join(pack_acc(a) for a in accs))
    assert not ok and each == [i != 20 for i in range(N)]
    assert HPA.ipa_decide_all(batch["dk"], b"") == (True, [])


@pytest.mark.parametrize("zk", [True, False])
def test_accumulation_prover_and_verifier_equal_the_oracle(HPA, batch, on_pallas, zk):
    rnd = random.Random("as-%d" % zk)
    rand = [rnd.randrange(PA.R) for _ in range(3 + (1 << K) + 1)] if zk else []
    it = iter(rand)
    pk = I.IpaProvingKey(K, batch["g"], batch["h"], batch["s"] if zk else None)
    m = 5
    t = T.Blake2bTranscript(PA)
    new = I.ipa_as_create_proof(pk, batch["accs"][:m], t, lambda: next(it))
    want_proof = t.finalize()
    assert next(it, None) is None  # the oracle drew exactly what the C API is handed
    dk = batch["dk"] if zk else batch["dk_nozk"]
    accs = batch["want"][:m * dk.acc_bytes]
    acc, proof = HPA.ipa_as_create_proof(dk, accs, b"".join(PA.fe_to_bytes(x) for x in rand))
    assert proof == want_proof and acc == pack_acc(new)
    assert HPA.ipa_as_verify(dk, accs, proof) == (1, pack_acc(new))
    assert HPA.ipa_decide_all(dk, acc) == (True, [True])
    # the verifier: another set of accumulators, a changed proof, leftover bytes, too few scalars for the prover
    assert HPA.ipa_as_verify(dk, batch["want"][dk.acc_bytes:(m + 1) * dk.acc_bytes], proof)[0] == 0
    bad = bytearray(proof)
    bad[-1] ^= 1
    assert HPA.ipa_as_verify(dk, accs, bytes(bad))[0] == 0
    with pytest.raises(HPA.HostError) as e:
        HPA.ipa_as_verify(dk, accs, proof + b"\x00")
    assert e.value.code == HPA.ERR_TRAILING
    with pytest.raises(HPA.HostError) as e:
        HPA.ipa_as_verify(dk, accs[:dk.acc_bytes], proof)  # accumulation.rs:107: more than one instance
    assert e.value.code == HPA.ERR_PANIC
    if zk:
        with pytest.raises(HPA.HostError) as e:
            HPA.ipa_as_create_proof(dk, accs, b"".join(PA.fe_to_bytes(x) for x in rand[:-1]))
        assert e.value.code == HPA.ERR_PANIC


def test_aggregate_equals_the_oracle_and_rejects_a_tampered_proof(HPA, batch, on_pallas):
    rnd = random.Random("aggregate")
    rand = [rnd.randrange(PA.R) for _ in range(3 + (1 << K) + 1)]
    rb = b"".join(PA.fe_to_bytes(x) for x in rand)
    it = iter(rand)
    pk = I.IpaProvingKey(K, batch["g"], batch["h"], batch["s"])
    t = T.Blake2bTranscript(PA)
    new = I.ipa_as_create_proof(pk, batch["accs"], t, lambda: next(it))
    assert I.ipa_decide(batch["g"], new)
    for route in _routes(HPA):
        ok, acc, proof, tm = HPA.aggregate(batch["protocol"], batch["dk"], batch["ib"], batch["pb"], N, rb, 4, route, timings=True)
        assert ok and acc == pack_acc(new) and proof == t.finalize(), route
        assert tm["total"] > 0 and tm["total"] >= tm["read_proofs"]
    assert HPA.ipa_as_verify(batch["dk"], batch["want"], proof) == (1, acc)
    # one tampered proof: an evaluation changed by one
    bad = bytearray(batch["proofs"][7])
    bad[9 * 32] ^= 1
    ps = list(batch["proofs"])
    ps[7] = bytes(bad)
    for route in _routes(HPA):
        ok, _, _, tm = HPA.aggregate(batch["protocol"], batch["dk"], batch["ib"], HPA.pack_proofs(ps), N, rb, 4, route, timings=True)
        assert not ok
        # the timings are written on a reject too: the stages that ran, and the total
        assert tm["read_proofs"] > 0 and tm["succinct_verify"] > 0 and tm["accumulate"] == 0 and tm["decide"] == 0
        assert tm["total"] >= tm["read_proofs"] + tm["succinct_verify"]
    # n = 1: nothing to accumulate, the single accumulator is decided
    one = batch["dk"].acc_bytes
    ok, acc, proof = HPA.aggregate(batch["protocol"], batch["dk"], batch["pack_instances"](batch["insts"][0]),
                                   HPA.pack_proofs(batch["proofs"][:1]), 1)
    assert ok and acc == batch["want"][:one] and proof == b""
    # a key that decides nothing: the succinct checks pass, `decide` does not
    gb2 = b"".join(PA.g1_to_bytes(p) for p in batch["g"][:3] + [batch["g"][4]] + batch["g"][4:])
    dk2 = HPA.IpaDecidingKey(K, gb2, PA.g1_to_bytes(batch["h"]), PA.g1_to_bytes(batch["s"]))
    ok, acc, _ = HPA.aggregate(batch["protocol"], dk2, batch["pack_instances"](batch["insts"][0]), HPA.pack_proofs(batch["proofs"][:1]), 1)
    assert not ok and acc == batch["want"][:one]
    assert not HPA.plonk_verify(batch["protocol"], dk2, batch["ib"], batch["pb"], N)
    dk2.close()
