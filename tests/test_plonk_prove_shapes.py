"""CPU: the shape catalogue of tests/plonk_prover_util.py (SHAPES), the reference of tests/test_gpu_plonk_prove_shapes.py.
For every shape, under Gwc19 over the EVM transcript and Bdfg21 over Poseidon, the model prover gives the catalogued outcome:

  proof               the oracle's verifier accepts the bytes, and rejects them with one byte flipped
  tail                h has coefficients from num_chunk * n on
  identity            nothing is left for the tail check (num_chunk n = N) and numerator(z) != Q(z) (z^n - 1): the model refuses,
                      and the bytes it would have written are rejected by the oracle's verifier -- the model without its
                      identity check wrote them
  transcript@...      the transcript refuses an identity commitment, in the stated phase or among the chunks
  missing_query       the numerator names an evaluation the protocol does not list

Then what the session computes of a protocol without a device: `host_plonk_prove.plan` (e, the columns, the bytes) and the
compiled numerator's extra columns and constants (hd_plonk_compile).  Last, the catalogue itself: all four combinations of
the extra columns, every extension from 0 to 3, every outcome."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hostfmt  # noqa: E402
import plonk_prover_util as PU  # noqa: E402
import plonk_synth as S  # noqa: E402

PAIRS = [(PU.GWC19, "evm"), (PU.BDFG21, "poseidon")]
# proof bytes (Gwc19 / EVM, Bdfg21 / Poseidon) where the points, sets and evaluations were counted by hand
SIZES = {"bare": (416, 288), "no_q_query": (416, 288), "deg3_two_chunks": (576, 384), "deg5_e3": (896, 576), "rot_wrap": (416, 256),
         "eval_lists": (448, 288), "bare_full_bad": (480, 320)}


@pytest.fixture(scope="module")
def lib():
    return hostfmt.load_host_lib()


def n_constants(e, seen=None):
    """the entries of the compiled constant table: one per distinct constant (Negated subtracts from a shared zero, Scaled
    multiplies by one) and one per challenge"""
    top = seen is None
    seen = set() if top else seen
    tag = e[0]
    if tag == "const":
        seen.add(("c", e[1] % PU.R))
    elif tag == "challenge":
        seen.add(("ch", e[1]))
    elif tag == "neg":
        seen.add(("c", 0))
        n_constants(e[1], seen)
    elif tag == "scaled":
        seen.add(("c", e[2] % PU.R))
        n_constants(e[1], seen)
    elif tag in ("sum", "prod"):
        n_constants(e[1], seen)
        n_constants(e[2], seen)
    elif tag == "dpow":
        for x in list(e[1]) + [e[2]]:
            n_constants(x, seen)
    return len(seen) if top else None


@pytest.mark.parametrize("mos,transcript", PAIRS)
@pytest.mark.parametrize("name", sorted(PU.SHAPES))
def test_the_model_gives_the_catalogued_outcome(name, mos, transcript):
    s = PU.SHAPES[name]
    pr, n = s.protocol, s.n
    n_chunk = pr["quotient"]["num_chunk"]
    assert s.outcome in PU.OUTCOMES
    if s.outcome.startswith("transcript@"):
        with pytest.raises(PU.T.TranscriptError) as e:
            PU.model_proof(s, mos, transcript)
        assert e.value.stage == s.outcome.split("@")[1]
        return
    if s.outcome == "missing_query":
        with pytest.raises(PU.P.ProtocolError, match="Missing query"):
            PU.model_proof(s, mos, transcript)
        return
    proof, info = PU.model_proof(s, mos, transcript)
    h = info["h"]
    assert len(h) == n << PU.extension(pr["quotient"]["numerator"])
    if s.outcome == "proof":
        assert proof is not None and "refused_by" not in info
        assert not any(h[n_chunk * n:]) and any(h[(n_chunk - 1) * n:n_chunk * n])
        assert PU.oracle_accepts(pr, s.instances, proof, mos, transcript)
        if name in SIZES:
            assert len(proof) == SIZES[name][PAIRS.index((mos, transcript))]
        flipped = bytearray(proof)
        flipped[len(proof) // 2] ^= 1
        try:
            assert not PU.oracle_accepts(pr, s.instances, bytes(flipped), mos, transcript)
        except (PU.T.TranscriptError, AssertionError, ValueError):
            pass  # the reader refuses the bytes: a rejection too
    elif s.outcome == "tail":
        assert proof is None and info["refused_by"] == "tail" and any(h[n_chunk * n:])
        if name == "tail_zero_chunk":  # the chunk is the identity: only the order of the two verdicts tells them apart
            assert not any(h[:n]) and n_chunk == 1
    else:
        assert s.outcome == "identity"
        assert proof is None and info["refused_by"] == "identity"
        assert len(h) == n_chunk * n and all(any(h[i * n:(i + 1) * n]) for i in range(n_chunk))  # the identity check stands alone
        assert not PU.oracle_accepts(pr, s.instances, info["unchecked_proof"], mos, transcript)
        if name in SIZES:
            assert len(info["unchecked_proof"]) == SIZES[name][PAIRS.index((mos, transcript))]


@pytest.mark.parametrize("name", sorted(PU.SHAPES))
def test_plan_and_compiled_numerator(lib, name):
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP
    from test_plonk_compile_model import compile_

    s = PU.SHAPES[name]
    pr, n = s.protocol, s.n
    num = pr["quotient"]["numerator"]
    l0_col, x_col, first_poly, e = s.expect
    assert e == PU.extension(num)
    n_wit = sum(nw for nw, _ in zip(pr["num_witness"], pr["num_challenge"]))
    n_polys = len(pr["preprocessed"]) + len(pr["num_instance"]) + n_wit
    n_cols, n_ext = first_poly + n_polys, n << e
    p = HP.plan(H.Protocol(S.pack_protocol(pr)))
    assert (p["e"], p["n_cols"], p["n_consts"]) == (e, n_cols, n_constants(num))
    assert p["bytes"] == 32 * ((n_cols + 1) * n + n_cols * n_ext + n_ext)  # cols_total = n_cols + the quotient's slot
    c = compile_(lib, pr, True)
    assert (c["l0_col"], c["x_col"], c["first_poly"], len(c["consts"])) == (l0_col, x_col, first_poly, n_constants(num))
    assert (c["e"], c["degree"], c["n_cols"]) == (e, PU.degree(num), n_cols)
    assert first_poly == (l0_col >= 0) + (x_col >= 0)
    assert pr["quotient"]["num_chunk"] * n <= n_ext


def test_the_catalogue_covers_what_it_claims():
    shapes = PU.SHAPES.values()
    assert {(s.expect[0] >= 0, s.expect[1] >= 0) for s in shapes} == {(False, False), (False, True), (True, False), (True, True)}
    assert {s.expect[3] for s in shapes} == {0, 1, 2, 3}
    assert {s.outcome for s in shapes} == set(PU.OUTCOMES)
    assert n_constants(PU.SHAPES["bare"].protocol["quotient"]["numerator"]) == 0  # an empty constant table goes to the device
    assert {s.k for s in shapes} >= {1, 3, 9, 10}
    # the empty tail, a tail of one chunk and longer ones
    tails = {(s.n << s.expect[3]) // s.n - s.protocol["quotient"]["num_chunk"] for s in shapes}
    assert {0, 1, 2, 4} <= tails
