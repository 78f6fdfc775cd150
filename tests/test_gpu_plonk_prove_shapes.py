"""GPU: the PLONK prover session (host/plonk_prover.hpp, csrc/plonk_prove.hip) at the shapes of tests/plonk_prover_util.py::SHAPES,
each there for a path circuits A and B do not take: no extra column, one of the two, no preprocessed polynomial, no instance,
an empty constant table, e = 0 .. 3, tails of 0, 1, 2 and 4 chunks, phases without witnesses or without challenges, repeated and
reordered evaluation lists, rotations that wrap, k = 1, 9 and 10.  The reference is the model prover of the util, pinned by the
oracle's verifier in tests/test_plonk_prove_shapes.py.

  * every shape with a proof: byte for byte the model's, accepted by the oracle and by snarkv_host_plonk_verify
  * every shape without one, through the raw calls with the outputs pre-filled: the tail check, the host's identity check where
    the tail is empty, an identity commitment in a phase and among the chunks, the late "Missing query"; a fresh session on
    the same context proves afterwards
  * two sessions alive at once on one context and on two; shapes alternating on one context; a session abandoned midway
  * k_plonk_tail_nonzero alone, against numpy.any: the block edge, the 2048-block cap and the strides past it, each word of a
    vector, a lane outside the first wave, the other bits of the status word, the words around the range"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plonk_prover_util as PU  # noqa: E402

pytestmark = pytest.mark.gpu
PAIRS = [(PU.GWC19, "evm"), (PU.BDFG21, "poseidon")]
PROVABLE = sorted(n for n, s in PU.SHAPES.items() if s.outcome == "proof")
REFUSED = sorted(n for n, s in PU.SHAPES.items() if s.outcome != "proof")
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


def prove(HP, ctx, name, mos, transcript):
    s = setup_of(name)
    return PU.prove(HP, ctx, s, mos, transcript, s.circuit.form)


def model(name, mos, transcript):
    return PU.model_proof(PU.SHAPES[name], mos, transcript)[0]


@pytest.mark.parametrize("mos,transcript", PAIRS)
@pytest.mark.parametrize("name", PROVABLE)
def test_parity_at_every_shape(gpu_ctx, HP, host_dk, name, mos, transcript):
    s = setup_of(name)
    assert (s.d_pre is None) == (not s.circuit.pre_coeffs)
    plan = HP.plan(s.protocol)
    assert plan["e"] == s.circuit.expect[3]
    proof = prove(HP, gpu_ctx, name, mos, transcript)
    assert proof is not None
    PU.check_three_ways(host_dk, s, proof, mos, transcript)


@pytest.mark.parametrize("mos,transcript", PAIRS)
@pytest.mark.parametrize("name", REFUSED)
def test_refusals_at_every_shape(gpu_ctx, HP, name, mos, transcript):
    import torch

    from snark_verifier_amd import host_api as H

    s = setup_of(name)
    c, a, outcome = s.circuit, HP.api(), s.circuit.outcome
    out, n = ctypes.create_string_buffer(FILL, len(FILL)), ctypes.c_size_t(7)
    ch, nc = ctypes.create_string_buffer(FILL[:256], 256), ctypes.c_size_t(7)
    phases = list(zip(c.protocol["num_witness"], c.protocol["num_challenge"]))
    with s.session(HP, gpu_ctx, mos, transcript) as p:
        challenges, ended = [], False
        for ph, (_, want) in enumerate(phases):
            d = PU.phase_input(c, ph, challenges, c.form)
            torch.cuda.synchronize()
            rc = a.phase(p._h, HP._addr(d), c.form, ch, 8, ctypes.byref(nc))
            if outcome == "transcript@phase%d" % ph:
                assert rc == H.ERR_TRANSCRIPT and ch.raw == FILL[:256]  # no challenge was written
                assert a.phase(p._h, HP._addr(d), c.form, ch, 8, ctypes.byref(nc)) == H.ERR_ARG and "ended" in HP.last_error()
                assert nc.value == 0 and ch.raw == FILL[:256]
                ended = True
                break
            assert rc == 1 and nc.value == want
            challenges += [int.from_bytes(ch.raw[32 * i:32 * i + 32], "little") for i in range(want)]
        rc = a.finish(p._h, out, len(out), ctypes.byref(n))
        if ended:
            assert rc == H.ERR_ARG and "ended" in HP.last_error()
        elif outcome in ("tail", "identity"):
            assert rc == 0 and HP.last_error() == HP.UNSATISFIED == PU.REFUSAL
        elif outcome == "transcript@finish":
            assert rc == H.ERR_TRANSCRIPT
        else:
            assert outcome == "missing_query"
            assert rc == H.ERR_INVALID_PROTOCOL and "Missing query" in HP.last_error()
        assert n.value == 0 and out.raw == FILL
        assert a.finish(p._h, out, len(out), ctypes.byref(n)) == H.ERR_ARG and "ended" in HP.last_error()  # a closed session
        assert n.value == 0 and out.raw == FILL
    # the context and its scratch are as good as before
    assert prove(HP, gpu_ctx, "bare", mos, transcript) == model("bare", mos, transcript)


def _interleaved(HP, ctx_a, ctx_b):
    import torch

    (name_a, mos_a, tr_a), (name_b, mos_b, tr_b) = ("deg5_e3", PU.GWC19, "evm"), ("only_x", PU.BDFG21, "poseidon")
    sa, sb = setup_of(name_a), setup_of(name_b)
    with sa.session(HP, ctx_a, mos_a, tr_a) as pa, sb.session(HP, ctx_b, mos_b, tr_b) as pb:
        da, db = PU.phase_input(sa.circuit, 0, [], PU.FORM_COEFFS), PU.phase_input(sb.circuit, 0, [], PU.FORM_COEFFS)
        torch.cuda.synchronize()
        assert pa.phase(da) == [] and pb.phase(db) == []
        got_b = pb.finish()
        got_a = pa.finish()
    assert got_a == model(name_a, mos_a, tr_a) and got_b == model(name_b, mos_b, tr_b)


def test_sessions_interleaved_on_one_context(gpu_ctx, HP):
    import snark_verifier_amd as sv

    _interleaved(HP, gpu_ctx, gpu_ctx)
    other = sv.Context(0)
    try:
        _interleaved(HP, gpu_ctx, other)
    finally:
        other.close()


def test_alternating_shapes_leave_nothing_behind(gpu_ctx, HP):
    mos, transcript = PU.GWC19, "evm"
    got = [(name, prove(HP, gpu_ctx, name, mos, transcript)) for name in ("deg5_e3", "bare", "deg5_e3", "e0_bad", "bare")]
    for name, proof in got:
        assert proof == model(name, mos, transcript), name
    assert got[3][1] is None and got[1][1] == got[4][1] and got[1][1] is not None


def test_a_session_abandoned_midway(gpu_ctx, HP):
    mos, transcript = PU.BDFG21, "evm"
    s = setup_of("phases")
    p = s.session(HP, gpu_ctx, mos, transcript)
    assert len(p.phase(None)) == 1  # the first phase: no witness, one challenge
    p.close()
    assert prove(HP, gpu_ctx, "phases", mos, transcript) == model("phases", mos, transcript)


# ---------------------------------------------------------------- the kernel alone
BLOCK_VECS, MAX_BLOCKS = 256, 2048
GRID_VECS = BLOCK_VECS * MAX_BLOCKS  # 524 288 vectors: past it the grid strides
COUNTS = [1, 127, 128, 129, GRID_VECS // 2, GRID_VECS // 2 + 1, 3 * (GRID_VECS // 2) + 5]


def _tail_cases(count):
    """[(word index, bit)]: where one bit is set, the buffer zero otherwise"""
    vecs, words = 2 * count, 8 * count
    mid = vecs // 2
    cases = [(0, 1), (words - 1, 1 << 31)] + [(4 * mid + j, 1 << (7 * j + 3)) for j in range(4)]
    off_lane = 64 + 37  # the second wave of the first block, lane 37
    if vecs > off_lane:
        cases.append((4 * off_lane + 2, 1 << 16))
    if vecs > GRID_VECS:  # read in a later step of the loop
        cases.append((4 * (vecs - 1) + 1, 1 << 9))
    if vecs > 2 * GRID_VECS + 165:
        cases += [(4 * (GRID_VECS + off_lane) + 3, 1 << 30), (4 * (2 * GRID_VECS + 165), 2)]
    assert all(0 <= w < words for w, _ in cases)
    return cases


@pytest.mark.parametrize("count", COUNTS)
def test_the_tail_kernel(gpu_ctx, count):
    import numpy as np
    import torch

    import snark_verifier_amd as sv

    lib = sv.load_library()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    check, upload = lib.snarkv_plonk_tail_check_dev, lib.snarkv_plonk_session_upload
    check.restype, check.argtypes = ctypes.c_int, [vp, vp, sz, vp]
    upload.restype, upload.argtypes = ctypes.c_int, [vp, vp, vp, sz]
    cases = [None] + _tail_cases(count)  # None: all zero
    lead = 64
    d_buf = torch.zeros(lead + 32 * count + 64, dtype=torch.uint8, device="cuda")
    d_buf[lead - 32] = 0x5A  # 32 bytes before the range
    d_buf[lead + 32 * count] = 0x5A  # just after it
    d_status = torch.full((len(cases),), 0xA0, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    base = d_buf.data_ptr() + lead
    assert base % 16 == 0
    host = np.zeros(8 * count, dtype=np.uint32)
    want = []
    zero = ctypes.c_uint32(0)
    for i, case in enumerate(cases):  # everything on the context's stream, in order
        status = d_status.data_ptr() + 4 * i
        if case is None:
            want.append(0xA0 | int(np.any(host)))
            assert check(gpu_ctx._h, base, count, status) == 0
            continue
        word, bit = case
        host[word] = bit
        want.append(0xA0 | int(np.any(host)))
        host[word] = 0
        value = ctypes.c_uint32(bit)
        assert upload(gpu_ctx._h, base + 4 * word, ctypes.byref(value), 4) == 0
        assert check(gpu_ctx._h, base, count, status) == 0
        assert upload(gpu_ctx._h, base + 4 * word, ctypes.byref(zero), 4) == 0
    gpu_ctx.sync()
    assert want == [0xA0] + [0xA1] * (len(cases) - 1)
    assert d_status.cpu().tolist() == want
    back = d_buf.cpu().numpy()
    assert back[lead - 32] == 0x5A and back[lead + 32 * count] == 0x5A and not back[lead:lead + 32 * count].any()
