"""CPU: the model prover of the PLONK-over-IPA session (tests/plonk_prover_pallas_util.py) against the oracle alone.  Its proofs
are what the GPU tests hold the device's bytes against, so they are checked here first: `plonk_proof_read(..., "bgh19")`,
`succinct_verify_ipa` and `ipa_decide` of the oracle accept them with no byte left over, for circuit A at k = 4, circuit B at
its smallest k and the bare shapes; the broken witnesses give no proof; and the consequences of blinds hold on integers
-- a zero polynomial with a non-zero blind is written, a zero blind on the zero top chunk is the transcript's refusal."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as BN  # noqa: E402
import plonk as P  # noqa: E402
import plonk_prover_pallas_util as PP  # noqa: E402


@pytest.fixture(scope="module")
def circuits():
    return {"A": PP.CircuitA(4), "A0": PP.CircuitA(4, zero_blinds=True), "B": PP.CircuitB(PP.CircuitB.MIN_K), "k1": PP.Bare(1),
            "full": PP.Bare(3, num_chunk=2), "zerocol": PP.Bare(3, zero_column=True)}


@pytest.mark.parametrize("name", ["A", "A0", "B", "k1", "full", "zerocol"])
def test_the_oracle_accepts_the_model_proofs(circuits, name):
    c = circuits[name]
    proof, info = PP.model_proof(c)
    assert proof is not None and len(proof) == PP.proof_length(c)
    acc = PP.oracle_accepts(c, proof)
    assert acc is not None and len(acc[0]) == c.k
    assert not any(info["h"][c.protocol["quotient"]["num_chunk"] * c.n:])
    flipped = bytearray(proof)
    flipped[len(proof) // 2] ^= 1
    assert PP.oracle_accepts(c, bytes(flipped)) is None
    assert PP.oracle_accepts(c, proof + b"\x00") is None  # a byte left over
    assert P.R == BN.R  # the oracle stack is BN254's again


def test_the_shapes_are_what_the_gpu_tests_take_them_for(circuits):
    a, b = circuits["A"], circuits["B"]
    assert PP.extension(a.protocol["quotient"]["numerator"]) == 2 and PP.extension(b.protocol["quotient"]["numerator"]) == 2
    assert b.k == 4 and 0 in b.protocol["num_witness"]
    assert {rot for _, rot in b.protocol["queries"]} == {-6, -1, 0, 1}
    assert PP.proof_length(b) > PP.proof_length(a)  # more than one query set more
    full = circuits["full"]
    assert full.protocol["quotient"]["num_chunk"] * full.n == full.n << PP.extension(full.protocol["quotient"]["numerator"])
    _, info = PP.model_proof(full)
    assert not any(info["h"][full.n:])  # the top chunk is zero: only its blind keeps the commitment off the identity
    _, info = PP.model_proof(circuits["zerocol"])
    assert not any(info["polys"][1]) and not any(info["polys"][2]) and not any(info["h"])
    assert all(x == 0 for x in circuits["A0"].chunk_blinds + circuits["A0"].pre_blinds + [circuits["A0"].opening_randomness[0]])


@pytest.mark.parametrize("bad", ["gate", "copy"])
def test_broken_witnesses_give_no_proof(bad):
    proof, info = PP.model_proof(PP.CircuitA(4, bad=bad))
    assert proof is None and info["refused_by"] == "tail"


def test_bare_refusals():
    proof, info = PP.model_proof(PP.Bare(3, bad=True))
    assert proof is None and info["refused_by"] == "tail"
    proof, info = PP.model_proof(PP.Bare(3, num_chunk=2, bad=True))  # no tail to show: the identity at z alone
    assert proof is None and info["refused_by"] == "identity"
    with pytest.raises(PP.TranscriptRefusal) as e:
        PP.model_proof(PP.Bare(3, num_chunk=2, top_blind_zero=True))
    assert e.value.stage == "finish" and "infinity" in str(e.value)
