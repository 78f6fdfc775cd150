"""CPU: the model prover of tests/plonk_prover_util.py, the reference of the GPU tests of the PLONK prover, against the
oracle's verifier: its proofs of circuit A at k = 4 and of circuit B at k = 6 pass `plonk_proof_read` + `succinct_verify` with
lhs = [s] rhs, for both multi-open schemes over both transcripts; for the two broken witnesses of circuit A the quotient has a
tail and no proof comes out."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plonk_prover_util as PU  # noqa: E402

_CIRCUITS = {}


def circuit(name):
    if name not in _CIRCUITS:
        _CIRCUITS[name] = PU.CircuitA(4) if name == "A" else PU.CircuitB(6)
    return _CIRCUITS[name]


@pytest.mark.parametrize("transcript", ["evm", "poseidon"])
@pytest.mark.parametrize("mos", [PU.GWC19, PU.BDFG21])
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_models_proofs_verify(name, mos, transcript):
    c = circuit(name)
    proof, info = PU.model_proof(c, mos, transcript)
    n, n_chunk = c.n, c.protocol["quotient"]["num_chunk"]
    assert proof is not None and not any(info["h"][n_chunk * n:]) and any(info["h"][(n_chunk - 1) * n:n_chunk * n])
    assert PU.oracle_accepts(c.protocol, c.instances, proof, mos, transcript)
    flipped = bytearray(proof)
    flipped[len(proof) // 2] ^= 1
    try:
        assert not PU.oracle_accepts(c.protocol, c.instances, bytes(flipped), mos, transcript)
    except (PU.T.TranscriptError, AssertionError, ValueError):
        pass  # the reader refuses the bytes: a rejection too


def test_a_wrong_instance_is_rejected():
    c = circuit("A")
    proof, _ = PU.model_proof(c, PU.GWC19, "evm")
    assert not PU.oracle_accepts(c.protocol, [[(c.instances[0][0] + 1) % PU.R]], proof, PU.GWC19, "evm")


@pytest.mark.parametrize("bad", ["gate", "copy"])
def test_a_broken_witness_leaves_a_tail(bad):
    c = PU.CircuitA(4, bad=bad)
    proof, info = PU.model_proof(c, PU.GWC19, "evm")
    assert proof is None and any(info["h"][3 * c.n:])
