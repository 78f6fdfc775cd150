"""CPU: the model prover of tests/plonk_prover_pallas_ci_util.py (the PLONK prover session on pallas with committed instances,
on Python integers) makes proofs that the oracle's reader, succinct verifier and decider accept, at every shape of the
instance columns the GPU test holds the device against: circuit A with its instance queried at rotation 0, circuit B at
rotations 0 and -1, two columns of 3 and 1 entries, a column over the whole Lagrange basis, an empty column (its commitment is
s), and a key without a constant.  The bases are the first points of the key's Lagrange basis, made by tests/g1_ntt_util.py's
inverse transform; over other bases the oracle rejects.  Without a key the model is the plain session's, byte for byte."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plonk_prover_pallas_ci_util as CI  # noqa: E402
import plonk_prover_pallas_util as PP  # noqa: E402

K = 4
NAMES = ["A", "B", "two-columns", "whole-basis", "empty-column", "no-constant"]


@pytest.fixture(scope="module")
def shapes():
    s = CI.shapes(K)
    assert sorted(s) == sorted(NAMES)
    return s


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_accepts_the_models_proof(shapes, name):
    c = shapes[name]
    proof, info = CI.model_proof(c)
    assert proof is not None, info.get("refused_by")
    assert len(proof) == CI.proof_length(c)
    assert CI.oracle_accepts(c, proof) is not None
    bad = bytearray(proof)
    bad[40] ^= 1
    assert CI.oracle_accepts(c, bytes(bad)) is None


def test_the_shapes_are_the_ones_named(shapes):
    n = 1 << K
    pr = {k: v.protocol for k, v in shapes.items()}
    assert pr["two-columns"]["num_instance"] == [3, 1] and len(pr["two-columns"]["instance_committing_key"]["bases"]) == 3
    assert pr["whole-basis"]["num_instance"] == [n] and len(pr["whole-basis"]["instance_committing_key"]["bases"]) == n
    assert pr["empty-column"]["num_instance"] == [0] and pr["no-constant"]["instance_committing_key"]["constant"] is None
    assert any(shapes["no-constant"].instances[0])
    inst_b = len(pr["B"]["preprocessed"])
    assert (inst_b, 0) in pr["B"]["queries"] and (inst_b, -1) in pr["B"]["queries"]
    with CI.on_pallas():
        sets = CI.PP.K.bdfg21_query_sets([(p, pr["B"]["domain"].rotate_scalar(1, rot), 0) for p, rot in pr["B"]["queries"]])
    assert sum(1 for s in sets if inst_b in s["polys"]) == 1 and len(sets) > 1  # one set holds it, at both rotations
    for c in shapes.values():
        key = c.protocol["instance_committing_key"]
        assert key["bases"] == CI.lagrange_basis(c.key)[:len(key["bases"])] and key["constant"] in (None, c.key.s)


def test_the_commitment_of_an_empty_column_is_s(shapes):
    c = shapes["empty-column"]
    assert c.key.commit([0] * c.n, 1) == c.key.s


def test_over_other_bases_the_oracle_rejects(shapes):
    c = CI.copy.copy(shapes["two-columns"])
    c.protocol = dict(c.protocol)
    key = c.protocol["instance_committing_key"]
    c.protocol["instance_committing_key"] = {"bases": list(c.key.g[:len(key["bases"])]), "constant": key["constant"]}  # g itself
    proof, _ = CI.model_prove(c)  # the prover commits over g as ever; the verifier recomputes over the bases
    assert proof is not None and CI.oracle_accepts(c, proof) is None


def test_without_a_key_the_model_is_the_plain_sessions():
    for c in (PP.CircuitA(K), PP.Bare(1)):
        assert CI.model_prove(c)[0] == PP.model_proof(c)[0] is not None
    plain = CI.Inst(K, [CI._column(K, 2, "z")], key=False)
    proof, _ = CI.model_prove(plain)
    assert proof == PP.model_prove(plain)[0] and CI.oracle_accepts(plain, proof) is not None


def test_an_all_zero_column_without_a_constant_is_the_transcripts_refusal():
    c = CI.Inst(K, [[0, 0]], constant=False, name="inst-zero-column-noconst")
    with pytest.raises(CI.TranscriptRefusal) as e:
        CI.model_prove(c)
    assert str(e.value).startswith("begin") and "infinity" in str(e.value)
