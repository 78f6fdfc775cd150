"""GPU: a PLONK prover session that takes the quotient one coset at a time (SNARKV_HOST_PLONK_QUOTIENT_COSETS of
include/snarkv_host_plonk_prove_opts.h, `flags=` of snark_verifier_amd.host_plonk_prove) against the session without the flag,
at entries of tests/plonk_prover_util.py::SHAPES: every return code, every challenge, every message and every proof byte of
the two sessions are equal, on Gwc19 and on Bdfg21 -- proofs, the tail's and the identity's 0 verdict, the transcript's refusal
of a zero chunk, the late "Missing query".  The calls are the raw ones with the outputs pre-filled, so that what a refusal
leaves in them is compared too.  `plan` reports the smaller allocation, the flagged proofs of two shapes pass the project's
verifier, and an unknown flag bit is refused."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plonk_prover_util as PU  # noqa: E402
import plonk_synth as S  # noqa: E402

pytestmark = pytest.mark.gpu
PAIRS = [(PU.GWC19, "evm"), (PU.BDFG21, "poseidon")]
NAMES = ["bare", "both_extras", "instances_3_1", "e0_zero", "deg3_two_chunks", "deg5_e3", "deg5_all8", "bare_k1", "bare_k10_values",
         "phases", "rot_wrap", "rot_extremes", "bare_bad", "tail_zero_chunk", "bare_full_bad", "missing_query"]
FILL = b"\xa5" * 4096


@pytest.fixture(scope="module")
def HP():
    from snark_verifier_amd import host_plonk_prove

    return host_plonk_prove


@pytest.fixture(scope="module")
def host_dk():
    from snark_verifier_amd import host_api as H

    key = H.DecidingKey(*PU.dk_bytes())
    yield key
    key.close()


_SETUPS = {}


def setup_of(name):
    if name not in _SETUPS:
        _SETUPS[name] = PU.Setup(PU.SHAPES[name])
    return _SETUPS[name]


def trace(HP, ctx, name, mos, transcript, flags):
    """one whole session through the raw calls -> everything it returned and wrote: per phase (rc, n_challenges, the challenge
    buffer, the message of a refusal), then finish's (rc, proof_len, the proof buffer, the message)"""
    import torch

    s = setup_of(name)
    c, a = s.circuit, HP.api()
    out, n = ctypes.create_string_buffer(FILL, len(FILL)), ctypes.c_size_t(7)
    seen = []
    p = HP.PlonkProver(s.protocol, ctx, s.d_srs, s.d_pre, c.instances, PU.MOS_ID[mos], PU.TRANSCRIPT_ID[transcript], flags=flags)
    with p:
        challenges = []
        for ph, want in enumerate(c.protocol["num_challenge"]):
            ch, nc = ctypes.create_string_buffer(FILL[:256], 256), ctypes.c_size_t(7)
            d = PU.phase_input(c, ph, challenges, c.form)
            torch.cuda.synchronize()
            rc = a.phase(p._h, HP._addr(d), c.form, ch, 8, ctypes.byref(nc))
            seen.append(("phase", rc, nc.value, ch.raw, HP.last_error() if rc != 1 else ""))
            if rc != 1:
                break
            challenges += [int.from_bytes(ch.raw[32 * i:32 * i + 32], "little") for i in range(want)]
        rc = a.finish(p._h, out, len(out), ctypes.byref(n))
        seen.append(("finish", rc, n.value, out.raw, HP.last_error() if rc != 1 else ""))
    return seen


@pytest.mark.parametrize("mos,transcript", PAIRS)
@pytest.mark.parametrize("name", NAMES)
def test_the_flagged_session_is_the_session(gpu_ctx, HP, name, mos, transcript):
    from snark_verifier_amd import host_api as H

    plain = trace(HP, gpu_ctx, name, mos, transcript, 0)
    flagged = trace(HP, gpu_ctx, name, mos, transcript, HP.QUOTIENT_COSETS)
    assert flagged == plain
    kind, rc, n, raw, msg = flagged[-1]
    outcome = PU.SHAPES[name].outcome
    assert kind == "finish"
    if outcome == "proof":
        assert rc == 1 and 0 < n < len(FILL) and raw[n:] == FILL[n:] and raw[:n] != FILL[:n]
    elif outcome in ("tail", "identity"):
        assert rc == 0 and msg == HP.UNSATISFIED and n == 0 and raw == FILL
    elif outcome == "transcript@finish":
        assert rc == H.ERR_TRANSCRIPT and n == 0 and raw == FILL
    else:
        assert outcome == "missing_query" and rc == H.ERR_INVALID_PROTOCOL and "Missing query" in msg and raw == FILL


@pytest.mark.parametrize("mos,transcript", PAIRS)
@pytest.mark.parametrize("name", ["bare", "deg5_e3"])
def test_flagged_proofs_pass_the_verifier(gpu_ctx, HP, host_dk, name, mos, transcript):
    from snark_verifier_amd import host_api as H

    s = setup_of(name)
    kind, rc, n, raw, _ = trace(HP, gpu_ctx, name, mos, transcript, HP.QUOTIENT_COSETS)[-1]
    assert rc == 1
    proof = raw[:n]
    inst = S.pack_instances(s.circuit.instances)
    assert H.plonk_verify(s.protocol, host_dk, inst, H.pack_proofs([proof]), 1, PU.MOS_ID[mos], PU.TRANSCRIPT_ID[transcript])
    assert proof == PU.model_proof(s.circuit, mos, transcript)[0]


@pytest.mark.parametrize("name", NAMES)
def test_plan_reports_the_smaller_allocation(HP, name):
    s = setup_of(name)
    plain, flagged = HP.plan(s.protocol), HP.plan(s.protocol, flags=HP.QUOTIENT_COSETS)
    n, n_ext = s.circuit.n, s.circuit.n << plain["e"]
    assert {k: v for k, v in plain.items() if k != "bytes"} == {k: v for k, v in flagged.items() if k != "bytes"}
    assert plain["bytes"] - flagged["bytes"] == 32 * plain["n_cols"] * (n_ext - n)
    assert (flagged["bytes"] < plain["bytes"]) == (plain["e"] > 0)


def test_an_unknown_flag_bit_is_refused(gpu_ctx, HP):
    from snark_verifier_amd import host_api as H

    s = setup_of("bare")
    for flags in (2, 3, 1 << 31):
        with pytest.raises(H.HostError) as err:
            HP.plan(s.protocol, flags=flags)
        assert err.value.code == H.ERR_ARG and "flag" in str(err.value)
        with pytest.raises(H.HostError) as err:
            HP.PlonkProver(s.protocol, gpu_ctx, s.d_srs, s.d_pre, s.circuit.instances, flags=flags)
        assert err.value.code == H.ERR_ARG and "flag" in str(err.value)
    assert trace(HP, gpu_ctx, "bare", PU.GWC19, "evm", 0)[-1][1] == 1  # the context is as good as before
