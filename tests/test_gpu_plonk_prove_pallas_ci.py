"""GPU: the PLONK prover session on pallas with committed instances (snark_verifier_amd.host_plonk_prove_pallas_ci,
include/snarkv_host_pallas_plonk_prove_ci.h) on the shapes of tests/plonk_prover_pallas_ci_util.py under a toy IPA key at k = 4.
Every proof is the model prover's, byte for byte (tests/test_plonk_model_pallas_ci.py pins the model with the oracle's
verifier), snarkv_host_pallas_plonk_verify accepts it -- the verifier recomputes the instance commitments over the protocol's
bases --, and `finish`'s accumulator is snarkv_host_pallas_plonk_succinct_verify_batch's.

  1  circuit A (instance queried at rotation 0), circuit B (rotations 0 and -1), two columns of 3 and 1 entries, a column over
     the whole basis, an empty column, a key without a constant
  2  circuit A as values, and with QUOTIENT_COSETS: the same bytes
  3  the whole-basis shape with its bases taken from snarkv_pallas_ipa_dk_lagrange_dev
  4  no constant and an all-zero column: SNARKV_HOST_ERR_TRANSCRIPT from begin
  5  wrong bases: a proof is written and the verifier rejects it
  6  a protocol without a key: the bytes of the old entry"""
import copy
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import g1_ntt_util as GU  # noqa: E402
import plonk_prover_pallas_ci_util as CI  # noqa: E402
import plonk_prover_pallas_util as PP  # noqa: E402

pytestmark = pytest.mark.gpu
K = 4
NAMES = ["A", "B", "two-columns", "whole-basis", "empty-column", "no-constant"]


@pytest.fixture(scope="module")
def HC():
    from snark_verifier_amd import host_plonk_prove_pallas_ci

    return host_plonk_prove_pallas_ci


@pytest.fixture(scope="module")
def HA():
    from snark_verifier_amd import host_api_pallas

    return host_api_pallas


@pytest.fixture(scope="module")
def shapes():
    return CI.shapes(K)


@pytest.fixture(scope="module")
def env(HA):
    """the context, the verifier's key and the setups made so far, closed at the end"""
    from snark_verifier_amd import pallas as PL

    ctx = PL.PallasContext(0)
    key = PP.key_of(K)
    e = {"ctx": ctx, "vk": HA.IpaDecidingKey(K, key.g_bytes, key.h_bytes, key.s_bytes), "setups": {}}
    yield e
    for s in e["setups"].values():
        s.close()
    e["vk"].close()
    ctx.close()


def setup_of(env, circuit):
    key = (circuit.name, circuit.k)
    if key not in env["setups"]:
        env["setups"][key] = CI.Setup(circuit, env["ctx"])
    return env["setups"][key]


def check_all_ways(HA, env, s, proof, acc):
    c = s.circuit
    want, _ = CI.model_proof(c)
    assert proof == want and len(proof) == CI.proof_length(c)
    packed = HA.pack_proofs([proof])
    assert HA.plonk_verify(s.protocol, env["vk"], s.inst, packed, 1)
    rc, accs = HA.plonk_succinct_verify_batch(s.protocol, env["vk"], s.inst, packed, 1)
    assert rc == 1 and accs == acc
    assert HA.ipa_decide_all(env["vk"], acc) == (True, [True])


@pytest.mark.parametrize("name", NAMES)
def test_every_shape_is_the_models_proof_and_verifies(env, HC, HA, shapes, name):
    s = setup_of(env, shapes[name])
    check_all_ways(HA, env, s, *CI.prove(HC, s, HC.FORM_COEFFS))


@pytest.mark.parametrize("flags", [0, 1])
def test_circuit_a_values_and_by_cosets(env, HC, HA, shapes, flags):
    assert flags in (0, HC.QUOTIENT_COSETS)
    s = setup_of(env, shapes["A"])
    check_all_ways(HA, env, s, *CI.prove(HC, s, HC.FORM_VALUES, flags))


def test_bases_made_by_the_device(env, HC, HA, shapes):
    """the protocol's bases are what snarkv_pallas_ipa_dk_lagrange_dev wrote for the resident key: the verifier accepts the
    proof over them"""
    import torch

    from snark_verifier_amd import g1_ntt

    base = shapes["whole-basis"]
    ctx, n = env["ctx"], base.n
    dk = ctx.ipa_dk_create(base.key.g_bytes)
    try:
        d_lag = torch.full((64 * n,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g1_ntt.dk_lagrange_dev(ctx, dk, d_lag)
        ctx.sync()
        made = GU.unpack("pallas", d_lag.cpu().numpy().tobytes())
    finally:
        dk.close()
    assert made == CI.lagrange_basis(base.key)
    c = copy.copy(base)
    c.protocol = dict(base.protocol, instance_committing_key={"bases": made, "constant": base.key.s})
    c.name = base.name + "-device-bases"
    s = setup_of(env, c)
    check_all_ways(HA, env, s, *CI.prove(HC, s, HC.FORM_COEFFS))


def test_an_identity_commitment_is_the_transcripts_refusal(env, HC, HA):
    c = CI.Inst(K, [[0, 0]], constant=False, name="inst-zero-column-noconst")
    s = setup_of(env, c)
    with pytest.raises(HA.HostError) as e:
        s.session(HC)
    assert e.value.code == HA.ERR_TRANSCRIPT
    with pytest.raises(CI.TranscriptRefusal):
        CI.model_prove(c)


def test_over_wrong_bases_a_proof_is_written_and_rejected(env, HC, HA, shapes):
    base = shapes["two-columns"]
    c = copy.copy(base)
    key = base.protocol["instance_committing_key"]
    c.protocol = dict(base.protocol, instance_committing_key={"bases": list(base.key.g[:len(key["bases"])]), "constant": key["constant"]})
    c.name = base.name + "-wrong-bases"
    s = setup_of(env, c)
    proof, acc = CI.prove(HC, s, HC.FORM_COEFFS)
    assert proof is not None and proof == CI.model_proof(c)[0] and len(proof) == CI.proof_length(c)
    assert not HA.plonk_verify(s.protocol, env["vk"], s.inst, HA.pack_proofs([proof]), 1)
    assert CI.oracle_accepts(c, proof) is None


def test_without_a_key_the_bytes_are_the_old_entrys(env, HC, HA):
    from snark_verifier_amd import host_plonk_prove_pallas as HP

    for c in (PP.CircuitA(K), CI.Inst(K, [CI._column(K, 2, "z")], key=False)):
        s = setup_of(env, c)
        new, old = CI.prove(HC, s, HC.FORM_COEFFS), PP.prove(HP, s, HP.FORM_COEFFS)
        assert new == old and new[0] == PP.model_prove(c)[0]
        assert HA.plonk_verify(s.protocol, env["vk"], s.inst, HA.pack_proofs([new[0]]), 1)
