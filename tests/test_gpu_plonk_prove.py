"""GPU: the PLONK prover session (snark_verifier_amd.host_plonk_prove, include/snarkv_host_plonk_prove.h) end to end on the
circuits of tests/plonk_prover_util.py under a toy SRS: the stages run against each other -- transforms, commitments,
transcript, quotient, evaluations, opening -- and every proof is checked three ways: it equals the bytes of the model prover
(pinned by the oracle's verifier in tests/test_plonk_prove_model.py), the oracle verifies it, and snarkv_host_plonk_verify
accepts it with the device decider.

  1  circuit A at k = 4, both schemes over both transcripts, the witness as coefficients
  2  circuit A at k = 8 (N = 1024: the transforms leave the single 512-element tile), the witness as values
  3  circuit B at k = 6, both schemes, its two Z made on the device by perm_product_dev between the phases from the challenges
     the session returned, the second chained to the first's value at the last row
  4  circuit A with a broken gate and with a broken copy: finish returns 0 with the message and no proof; only destroy is left
  5  one flipped byte of a proof of 1 is rejected
  6  argument errors and the capacity answers, with the session usable after each"""
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
R = PU.R


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


Setup, prove, check_three_ways, to_dev, pack_cols = PU.Setup, PU.prove, PU.check_three_ways, PU.to_dev, PU.pack_cols

_SETUPS = {}


def setup_of(name, k, bad=None):
    key = (name, k, bad)
    if key not in _SETUPS:
        _SETUPS[key] = Setup(PU.CircuitA(k, bad=bad) if name == "A" else PU.CircuitB(k))
    return _SETUPS[key]


@pytest.mark.parametrize("transcript", ["evm", "poseidon"])
@pytest.mark.parametrize("mos", [PU.GWC19, PU.BDFG21])
def test_circuit_a_coefficients(gpu_ctx, HP, host_dk, mos, transcript):
    s = setup_of("A", 4)
    proof = prove(HP, gpu_ctx, s, mos, transcript, HP.FORM_COEFFS)
    check_three_ways(host_dk, s, proof, mos, transcript)


@pytest.mark.parametrize("mos,transcript", [(PU.GWC19, "evm"), (PU.BDFG21, "poseidon")])
def test_circuit_a_values_past_one_tile(gpu_ctx, HP, host_dk, mos, transcript):
    s = setup_of("A", 8)
    assert HP.plan(s.protocol)["e"] == 2  # N = 2^10
    proof = prove(HP, gpu_ctx, s, mos, transcript, HP.FORM_VALUES)
    check_three_ways(host_dk, s, proof, mos, transcript)


@pytest.mark.parametrize("mos", [PU.GWC19, PU.BDFG21])
def test_circuit_b_with_z_made_on_the_device(gpu_ctx, HP, host_dk, mos):
    import torch

    from snark_verifier_amd import poly_prod as PP

    s = setup_of("B", 6)
    c = s.circuit
    n, u = c.n, c.u
    d_cols = to_dev(pack_cols([c.a, c.b, c.c] + c.ids + c.sigma))  # values: 0..2 the advice, 3..5 the identities, 6..8 sigma

    def phase_columns(ph, challenges):
        if ph == 0:
            return to_dev(pack_cols([c.a, c.b, c.c]))
        _, beta, gamma = challenges
        d_w = to_dev(pack_cols([[0] * n, [0] * n, c.random_values]))
        d_work = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        z1, z2 = d_w.data_ptr(), d_w.data_ptr() + 32 * n
        PP.perm_product_dev(gpu_ctx, d_cols, n, 9, [0, 1], [3, 4], [6, 7], beta, gamma, d_work, z1)
        PP.perm_product_dev(gpu_ctx, d_cols, n, 9, [2], [5], [8], beta, gamma, d_work, z2, d_start=z1 + 32 * u)
        gpu_ctx.sync()
        for j, blind in enumerate((c.blind_z1, c.blind_z2)):  # the rows past the last one carry the blinding values
            d_w[32 * (n * j + u + 1):32 * n * (j + 1)] = to_dev(PU.U.pack(blind))
        return d_w

    proof = prove(HP, gpu_ctx, s, mos, "evm", HP.FORM_VALUES, phase_columns)
    check_three_ways(host_dk, s, proof, mos, "evm")


@pytest.mark.parametrize("bad", ["gate", "copy"])
def test_a_broken_witness_gives_no_proof(gpu_ctx, HP, bad):
    import torch

    from snark_verifier_amd import host_api as H

    s = setup_of("A", 4, bad)
    c, a = s.circuit, HP.api()
    assert PU.model_proof(c, PU.GWC19, "evm")[0] is None
    with s.session(HP, gpu_ctx, PU.GWC19, "evm") as p:
        challenges = []
        for ph in range(2):
            d = to_dev(pack_cols(c.phase_coeffs(ph, list(challenges))))
            torch.cuda.synchronize()
            challenges += p.phase(d)
        out, n = ctypes.create_string_buffer(b"\xa5" * 4096, 4096), ctypes.c_size_t(7)
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == 0
        assert HP.last_error() == HP.UNSATISFIED == PU.REFUSAL and n.value == 0 and out.raw == b"\xa5" * 4096
        nc = ctypes.c_size_t(0)
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == H.ERR_ARG and n.value == 0
        assert a.phase(p._h, HP._addr(d), 0, out, 64, ctypes.byref(nc)) == H.ERR_ARG
    with s.session(HP, gpu_ctx, PU.GWC19, "evm") as p:  # the same through the wrapper: None
        challenges = []
        for ph in range(2):
            d = to_dev(pack_cols(c.phase_coeffs(ph, list(challenges))))
            torch.cuda.synchronize()
            challenges += p.phase(d)
        assert p.finish() is None


def test_one_flipped_byte_is_rejected(gpu_ctx, HP, host_dk):
    from snark_verifier_amd import host_api as H

    s = setup_of("A", 4)
    proof = prove(HP, gpu_ctx, s, PU.GWC19, "evm", HP.FORM_COEFFS)
    inst = check_three_ways(host_dk, s, proof, PU.GWC19, "evm")
    for at in (len(proof) - 1, 64 * 7 + 5):  # in the last opening point; in an evaluation
        bad = bytearray(proof)
        bad[at] ^= 1
        try:
            assert not H.plonk_verify(s.protocol, host_dk, inst, H.pack_proofs([bytes(bad)]), 1, 0, 0)
        except H.HostError as e:
            assert e.code == H.ERR_TRANSCRIPT  # the bytes no longer decode: a rejection by the reader


def test_argument_errors_and_capacity_leave_the_session_usable(gpu_ctx, HP, host_dk):
    import torch

    from snark_verifier_amd import host_api as H

    s = setup_of("A", 4)
    c, a = s.circuit, HP.api()
    want, _ = PU.model_proof(c, PU.BDFG21, "evm")
    out, n = ctypes.create_string_buffer(b"\xa5" * 4096, 4096), ctypes.c_size_t(0)
    ch = ctypes.create_string_buffer(32 * 4)
    with s.session(HP, gpu_ctx, PU.BDFG21, "evm") as p:
        d0 = to_dev(pack_cols(c.phase_coeffs(0, [])))
        torch.cuda.synchronize()
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == H.ERR_ARG and n.value == 0  # before the last phase
        assert a.phase(p._h, HP._addr(d0), 5, ch, 4, ctypes.byref(n)) == H.ERR_ARG and "form" in HP.last_error()
        assert a.phase(p._h, None, 0, ch, 4, ctypes.byref(n)) == H.ERR_ARG  # a phase with witnesses takes an address
        assert a.phase(p._h, HP._addr(d0), 0, ch, 4, None) == H.ERR_ARG
        assert a.phase(p._h, HP._addr(d0), 0, None, 4, ctypes.byref(n)) == H.ERR_ARG
        assert a.phase(p._h, HP._addr(d0), 0, ch, 1, ctypes.byref(n)) == H.ERR_CAPACITY and n.value == 2
        assert ch.raw == b"\x00" * 128
        challenges = p.phase(d0)
        assert len(challenges) == 2
        d1 = to_dev(pack_cols(c.phase_coeffs(1, list(challenges))))
        torch.cuda.synchronize()
        challenges += p.phase(d1)
        assert a.phase(p._h, HP._addr(d1), 0, ch, 4, ctypes.byref(n)) == H.ERR_ARG and "finish" in HP.last_error()  # no third phase
        assert a.finish(p._h, out, len(out), None) == H.ERR_ARG
        assert a.finish(p._h, out, len(want) - 1, ctypes.byref(n)) == H.ERR_CAPACITY and n.value == len(want)
        assert a.finish(p._h, None, 0, ctypes.byref(n)) == H.ERR_CAPACITY and n.value == len(want)
        assert out.raw == b"\xa5" * 4096
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == 1 and n.value == len(want)
        assert out.raw[:n.value] == want and out.raw[n.value:] == b"\xa5" * (4096 - n.value)
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == H.ERR_ARG and n.value == 0  # the session has ended
    inst = S.pack_instances(c.instances)
    assert H.plonk_verify(s.protocol, host_dk, inst, H.pack_proofs([want]), 1, 1, 0)
    # begin's own refusals that need a device: the instances do not fit the protocol
    with pytest.raises(H.HostError) as e:
        HP.PlonkProver(s.protocol, gpu_ctx, s.d_srs, s.d_pre, [[1, 2]], 0, 0)
    assert e.value.code == H.ERR_INVALID_INSTANCES
