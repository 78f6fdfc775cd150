"""GPU: the PLONK prover session on pallas (snark_verifier_amd.host_plonk_prove_pallas, include/snarkv_host_pallas_plonk_prove.h)
end to end on the circuits of tests/plonk_prover_pallas_util.py under a toy IPA key.  Every proof is held against the bytes of
the model prover (which tests/test_plonk_model_pallas.py pins with the oracle's verifier), the oracle verifies it,
snarkv_host_pallas_plonk_verify accepts it -- for the first time a proof made from a witness --, and the accumulator that
`finish` returns is the one snarkv_host_pallas_plonk_succinct_verify_batch computes for the proof.

  1  circuit A at k = 4 (n = 16, e = 2, three chunks), the witness as coefficients, random non-zero blinds
  2  the same with the witness as values, and with SNARKV_HOST_PLONK_QUOTIENT_COSETS: the same bytes
  3  the same with all blinds zero: the blinded commitment gives the plain one's bytes
  4  circuit B at k = 4: a phase without witnesses, rotations -6 and -1, several query sets in the opening
  5  a b + c at k = 1: a key of two points, an opening of one round
  6  num_chunk n = N: a non-zero blind on the zero top chunk gives a proof, a zero blind the transcript's refusal; zero witness
     polynomials with non-zero blinds are written
  7  broken witnesses return 0 with the message and no proof byte; a flipped byte of a good proof is rejected
  8  argument errors and the capacity answers, with the session usable after each; the caller's device buffers are unchanged"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plonk_prover_pallas_util as PP  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def HP():
    from snark_verifier_amd import host_plonk_prove_pallas

    return host_plonk_prove_pallas


@pytest.fixture(scope="module")
def HA():
    from snark_verifier_amd import host_api_pallas

    return host_api_pallas


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    ctx = PL.PallasContext(0)
    yield ctx
    for s in _SETUPS.values():
        s.close()
    _SETUPS.clear()
    for k in _HOST_KEYS.values():
        k.close()
    _HOST_KEYS.clear()
    ctx.close()


_SETUPS, _HOST_KEYS = {}, {}


def setup_of(pctx, circuit):
    key = (circuit.name, circuit.k)
    if key not in _SETUPS:
        _SETUPS[key] = PP.Setup(circuit, pctx)
    return _SETUPS[key]


def host_key(HA, k):
    if k not in _HOST_KEYS:
        key = PP.key_of(k)
        _HOST_KEYS[k] = HA.IpaDecidingKey(k, key.g_bytes, key.h_bytes, key.s_bytes)
    return _HOST_KEYS[k]


def check_all_ways(HA, s, proof, acc):
    """the model's bytes; the oracle accepts; plonk_verify accepts; the accumulator is succinct_verify_batch's and the oracle's"""
    c = s.circuit
    want, _ = PP.model_proof(c)
    assert proof == want and len(proof) == PP.proof_length(c)
    oracle_acc = PP.oracle_accepts(c, proof)
    assert oracle_acc is not None and acc == PP.pack_acc(oracle_acc)
    dk = host_key(HA, c.k)
    assert HA.plonk_verify(s.protocol, dk, s.inst, HA.pack_proofs([proof]), 1)
    rc, accs = HA.plonk_succinct_verify_batch(s.protocol, dk, s.inst, HA.pack_proofs([proof]), 1)
    assert rc == 1 and accs == acc
    assert HA.ipa_decide_all(dk, acc) == (True, [True])


def test_circuit_a_coefficients(pctx, HP, HA):
    s = setup_of(pctx, PP.CircuitA(4))
    assert HP.plan(s.protocol)["e"] == 2 and s.circuit.protocol["quotient"]["num_chunk"] == 3
    assert all(b != 0 for b in s.circuit.chunk_blinds + sum(s.circuit.phase_blinds, []))
    check_all_ways(HA, s, *PP.prove(HP, s, HP.FORM_COEFFS))


@pytest.mark.parametrize("flags", [0, 1])
def test_circuit_a_values_and_by_cosets(pctx, HP, HA, flags):
    s = setup_of(pctx, PP.CircuitA(4))
    assert flags in (0, HP.QUOTIENT_COSETS)
    check_all_ways(HA, s, *PP.prove(HP, s, HP.FORM_VALUES, flags))


def test_circuit_a_with_all_blinds_zero(pctx, HP, HA):
    import torch

    from snark_verifier_amd import ipa_batch as IB

    s = setup_of(pctx, PP.CircuitA(4, zero_blinds=True))
    c = s.circuit
    proof, acc = PP.prove(HP, s, HP.FORM_COEFFS)
    check_all_ways(HA, s, proof, acc)
    # the witness points in the proof are the plain commitments' bytes
    cols = c.phase_coeffs(0, [])
    d, d_out = PP.to_dev(PP.pack_cols(cols)), torch.zeros(64 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    IB.commit_batch_dev(pctx, s.dk, d.data_ptr(), c.n, 3, d_out.data_ptr())
    pctx.sync()
    plain = d_out.cpu().numpy().tobytes()
    for i in range(3):
        x, y = int.from_bytes(plain[64 * i:64 * i + 32], "little"), int.from_bytes(plain[64 * i + 32:64 * i + 64], "little")
        assert proof[32 * i:32 * i + 32] == (x | ((y & 1) << 255)).to_bytes(32, "little")


def test_circuit_b_smallest(pctx, HP, HA):
    s = setup_of(pctx, PP.CircuitB(PP.CircuitB.MIN_K))
    assert 0 in s.circuit.protocol["num_witness"] and {r for _, r in s.circuit.protocol["queries"]} == {-6, -1, 0, 1}
    check_all_ways(HA, s, *PP.prove(HP, s, HP.FORM_VALUES))


def test_the_smallest_protocol(pctx, HP, HA):
    s = setup_of(pctx, PP.Bare(1))
    assert s.dk.k == 1  # two points, one round
    proof, acc = PP.prove(HP, s, HP.FORM_COEFFS)
    assert len(proof) == 32 * (3 + 1 + 3) + 64 + 32 + 160 and len(acc) == 32 + 64
    check_all_ways(HA, s, proof, acc)


def test_blinds_and_the_identity(pctx, HP, HA):
    import torch

    # num_chunk n = N: the top chunk of h is zero, and its blind alone keeps the commitment off the identity
    s = setup_of(pctx, PP.Bare(3, num_chunk=2))
    c = s.circuit
    assert HP.plan(s.protocol)["e"] == 1 and 2 * c.n == c.n << 1 and c.chunk_blinds[1] != 0
    assert not any(PP.model_proof(c)[1]["h"][c.n:])
    check_all_ways(HA, s, *PP.prove(HP, s, HP.FORM_COEFFS))
    # ... with a zero blind on it: the transcript's refusal, no proof byte, and the session has ended
    s0 = setup_of(pctx, PP.Bare(3, num_chunk=2, top_blind_zero=True))
    c0, a = s0.circuit, HP.api()
    with pytest.raises(PP.TranscriptRefusal):
        PP.model_proof(c0)
    with s0.session(HP) as p:
        d = PP.to_dev(PP.pack_cols(c0.phase_coeffs(0, [])))
        torch.cuda.synchronize()
        assert p.phase(d, c0.phase_blinds[0]) == []
        out, acc = ctypes.create_string_buffer(b"\xa5" * 1024, 1024), ctypes.create_string_buffer(b"\xa5" * 160, 160)
        n = ctypes.c_size_t(7)
        f_blind, _, omega_bar = c0.opening_randomness
        args = (HP._blinds(c0.chunk_blinds), HP._fe(f_blind), HP._addr(s0.d_pbar), HP._fe(omega_bar))
        assert a.finish(p._h, *args, out, len(out), ctypes.byref(n), acc) == HA.ERR_TRANSCRIPT and "infinity" in HP.last_error()
        assert n.value == 0 and out.raw == b"\xa5" * 1024 and acc.raw == b"\xa5" * 160
        assert a.finish(p._h, *args, out, len(out), ctypes.byref(n), acc) == HA.ERR_ARG and "ended" in HP.last_error()
    # zero witness polynomials (and a zero h) with non-zero blinds are written
    sz = setup_of(pctx, PP.Bare(3, zero_column=True))
    assert not any(sz.circuit.phase_values(0, [])[1]) and all(sz.circuit.phase_blinds[0])
    check_all_ways(HA, sz, *PP.prove(HP, sz, HP.FORM_VALUES))
    # ... and with zero blinds they are the identity: refused in the phase
    with sz.session(HP) as p:
        d = PP.to_dev(PP.pack_cols(sz.circuit.phase_coeffs(0, [])))
        torch.cuda.synchronize()
        with pytest.raises(HA.HostError) as e:
            p.phase(d, [sz.circuit.phase_blinds[0][0], 0, 0])
        assert e.value.code == HA.ERR_TRANSCRIPT


@pytest.mark.parametrize("bad", ["gate", "copy"])
def test_a_broken_witness_gives_no_proof(pctx, HP, HA, bad):
    s = setup_of(pctx, PP.CircuitA(4, bad=bad))
    c, a = s.circuit, HP.api()
    assert PP.model_proof(c)[0] is None
    import torch

    with s.session(HP) as p:
        challenges = []
        for ph in range(2):
            d = PP.to_dev(PP.pack_cols(c.phase_coeffs(ph, list(challenges))))
            torch.cuda.synchronize()
            challenges += p.phase(d, c.phase_blinds[ph])
        out, acc = ctypes.create_string_buffer(b"\xa5" * 4096, 4096), ctypes.create_string_buffer(b"\xa5" * 192, 192)
        n = ctypes.c_size_t(7)
        f_blind, _, omega_bar = c.opening_randomness
        args = (HP._blinds(c.chunk_blinds), HP._fe(f_blind), HP._addr(s.d_pbar), HP._fe(omega_bar))
        assert a.finish(p._h, *args, out, len(out), ctypes.byref(n), acc) == 0
        assert HP.last_error() == HP.UNSATISFIED == PP.REFUSAL and n.value == 0 and out.raw == b"\xa5" * 4096
        assert a.finish(p._h, *args, out, len(out), ctypes.byref(n), acc) == HA.ERR_ARG and n.value == 0
    assert PP.prove(HP, s) == (None, None)  # the same through the wrapper


def test_one_flipped_byte_is_rejected(pctx, HP, HA):
    s = setup_of(pctx, PP.CircuitA(4))
    proof, _ = PP.prove(HP, s)
    dk = host_key(HA, 4)
    assert HA.plonk_verify(s.protocol, dk, s.inst, HA.pack_proofs([proof]), 1)
    for at in (len(proof) - 1, 32 * 5 + 5, 32 * 7 + 5, 32 * 18 + 3):  # in U; in a chunk's point; in an evaluation; in a q_eval
        bad = bytearray(proof)
        bad[at] ^= 1
        try:
            assert not HA.plonk_verify(s.protocol, dk, s.inst, HA.pack_proofs([bytes(bad)]), 1)
        except HA.HostError as e:
            assert e.code == HA.ERR_TRANSCRIPT  # the bytes no longer decode: a rejection by the reader


def test_argument_errors_and_capacity_leave_the_session_usable(pctx, HP, HA):
    import torch

    s = setup_of(pctx, PP.CircuitA(4))
    c, a = s.circuit, HP.api()
    want, _ = PP.model_proof(c)
    out, acc = ctypes.create_string_buffer(b"\xa5" * 4096, 4096), ctypes.create_string_buffer(32 * 4 + 64)
    n = ctypes.c_size_t(0)
    ch = ctypes.create_string_buffer(32 * 4)
    f_blind, _, omega_bar = c.opening_randomness
    fin = (HP._blinds(c.chunk_blinds), HP._fe(f_blind), HP._addr(s.d_pbar), HP._fe(omega_bar))
    with s.session(HP) as p:
        d0, b0 = PP.to_dev(PP.pack_cols(c.phase_coeffs(0, []))), HP._blinds(c.phase_blinds[0])
        torch.cuda.synchronize()
        assert a.finish(p._h, *fin, out, len(out), ctypes.byref(n), acc) == HA.ERR_ARG and n.value == 0  # before the last phase
        assert a.phase(p._h, HP._addr(d0), 5, b0, ch, 4, ctypes.byref(n)) == HA.ERR_ARG and "form" in HP.last_error()
        assert a.phase(p._h, None, 0, b0, ch, 4, ctypes.byref(n)) == HA.ERR_ARG  # a phase with witnesses takes an address
        assert a.phase(p._h, HP._addr(d0), 0, None, ch, 4, ctypes.byref(n)) == HA.ERR_ARG and "blinds" in HP.last_error()
        assert a.phase(p._h, HP._addr(d0), 0, b0, ch, 4, None) == HA.ERR_ARG
        assert a.phase(p._h, HP._addr(d0), 0, b0, None, 4, ctypes.byref(n)) == HA.ERR_ARG
        assert a.phase(p._h, ctypes.c_void_p(d0.data_ptr() + 8), 0, b0, ch, 4, ctypes.byref(n)) == HA.ERR_ARG
        assert a.phase(p._h, HP._addr(d0), 0, b0, ch, 1, ctypes.byref(n)) == HA.ERR_CAPACITY and n.value == 2
        assert ch.raw == b"\x00" * 128
        challenges = p.phase(d0, c.phase_blinds[0])
        assert len(challenges) == 2
        d1 = PP.to_dev(PP.pack_cols(c.phase_coeffs(1, list(challenges))))
        torch.cuda.synchronize()
        challenges += p.phase(d1, c.phase_blinds[1])
        assert a.phase(p._h, HP._addr(d1), 0, b0, ch, 4, ctypes.byref(n)) == HA.ERR_ARG and "finish" in HP.last_error()  # no third phase
        assert a.finish(p._h, *fin, out, len(out), None, acc) == HA.ERR_ARG
        assert a.finish(p._h, *fin, out, len(want) - 1, ctypes.byref(n), acc) == HA.ERR_CAPACITY and n.value == len(want)
        assert a.finish(p._h, None, None, None, None, None, 0, ctypes.byref(n), None) == HA.ERR_CAPACITY and n.value == len(want)
        for hole in range(4):  # each of the opening's inputs is required
            args = list(fin)
            args[hole] = None
            assert a.finish(p._h, *args, out, len(out), ctypes.byref(n), acc) == HA.ERR_ARG and n.value == 0
        assert a.finish(p._h, *fin, out, len(out), ctypes.byref(n), None) == HA.ERR_ARG
        assert out.raw == b"\xa5" * 4096
        assert a.finish(p._h, *fin, out, len(out), ctypes.byref(n), acc) == 1 and n.value == len(want)
        assert out.raw[:n.value] == want and out.raw[n.value:] == b"\xa5" * (4096 - n.value)
        assert acc.raw == PP.pack_acc(PP.oracle_accepts(c, want))
        assert a.finish(p._h, *fin, out, len(out), ctypes.byref(n), acc) == HA.ERR_ARG and n.value == 0  # the session has ended
    assert s.unchanged()  # preprocessed and p_bar are byte for byte what the caller gave
    # begin's own refusals with a device: a key of another size, a null h or s, instances that do not fit the protocol
    small = setup_of(pctx, PP.Bare(3))
    for kw in ({"dk": small.dk}, {"h": False}, {"s": False}):
        with pytest.raises(HA.HostError) as e:
            s.session(HP, **kw)
        assert e.value.code == HA.ERR_ARG, kw
    with pytest.raises(HA.HostError) as e:
        HP.PlonkProver(s.protocol, pctx, s.dk, c.key.h_bytes, c.key.s_bytes, s.d_pre, c.pre_blinds, [[1, 2]])
    assert e.value.code == HA.ERR_INVALID_INSTANCES
    check_all_ways(HA, s, *PP.prove(HP, s))  # and the context, the key and the setup still prove
