"""CPU: the C ABI of the PLONK prover (include/snarkv_host_plonk_prove.h in libsnarkv_host.so, and the device side it stands on,
include/snarkv_plonk_prove.h in libsnarkv_amd.so): the headers are strict C99, each library exports the names of its header and
no other library does, the ctypes table of snark_verifier_amd.host_plonk_prove lists exactly the host header's names and shares
none with snarkv_host.h's table, `plan` gives the compiled plan's numbers without a device and refuses what the prover refuses,
and every refusal that comes before device work returns its documented code."""
import copy
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HOST_HDR = os.path.join(INC, "snarkv_host_plonk_prove.h")
DEV_HDR = os.path.join(INC, "snarkv_plonk_prove.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402
import plonk_prover_util as PU  # noqa: E402
import plonk_synth as S  # noqa: E402

DEV_NAMES = sorted("snarkv_plonk_" + n for n in ("session_alloc", "session_free", "session_upload", "session_copy",
                                                 "session_download", "tail_check_dev"))


def test_headers_are_strict_c99():
    for h in (HOST_HDR, DEV_HDR):
        AU.assert_strict_c99(h)


def test_header_library_and_binding_agree():
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_kzg_open as HK
    from snark_verifier_amd import host_plonk_prove as HP
    from snark_verifier_amd import pallas as PL

    names = AU.declared(HOST_HDR, r"\b(snarkv_host_[a-z0-9_]+)\s*\(")
    assert names == sorted(HP.SIGNATURES) == sorted(HP.PREFIX + n for n in ("plan", "begin", "phase", "finish", "destroy"))
    assert not set(names) & set(H._SIGNATURES) and not set(names) & set(HK.SIGNATURES)
    a = HP.api()
    bn, pa = sv.load_library(), PL.load_library()
    for n in names:
        assert hasattr(a.lib, n) and not hasattr(bn, n) and not hasattr(pa, n), n
        fn = getattr(a, n[len(HP.PREFIX):])
        assert (fn.restype, fn.argtypes) == HP.SIGNATURES[n]
    assert AU.declared(DEV_HDR) == DEV_NAMES
    others = set()
    for mod, attr in AU.TABLES.items():
        others |= set(getattr(__import__("snark_verifier_amd." + mod, fromlist=[attr]), attr))
    assert not others & set(DEV_NAMES)
    for n in DEV_NAMES:
        assert hasattr(bn, n) and not hasattr(pa, n) and not hasattr(pa, n.replace("snarkv_", "snarkv_pallas_")), n
    assert callable(sv.host_plonk_prove.plan) and callable(sv.host_plonk_prove.PlonkProver)


def _protocol(pr):
    from snark_verifier_amd import host_api as H

    return H.Protocol(S.pack_protocol(pr))


def test_plan_without_a_device():
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP

    for circuit, k, n_cols in ((PU.CircuitA(4), 4, 12), (PU.CircuitB(6), 6, 17)):
        p = HP.plan(_protocol(circuit.protocol))
        assert (p["e"], p["n_cols"]) == (2, n_cols) and 0 < p["n_instr"] <= 4096 and 0 < p["n_consts"] <= 1024
        n, n_ext = 1 << k, 1 << (k + 2)
        assert p["bytes"] == 32 * ((n_cols + 1) * n + n_cols * n_ext + n_ext)  # the columns and the quotient's slot, work, h
    a = PU.CircuitA(4).protocol
    for change, word in (({"linearization": "WithoutConstant"}, "linearization"),
                         ({"queries": a["queries"] + [(5, 0)]}, "instance polynomial"),
                         ({"quotient": dict(a["quotient"], chunk_degree=2)}, "chunk_degree"),
                         ({"quotient": dict(a["quotient"], numerator=("lagrange", 600))}, "Lagrange"),
                         ({"domain": PU.P.Domain(27)}, "k + e")):
        pr = copy.copy(a)
        pr.update(change)
        with pytest.raises(H.HostError) as e:
            HP.plan(_protocol(pr))
        assert e.value.code == H.ERR_INVALID_PROTOCOL and word in str(e.value), change
    assert HP.api().plan(None, None, None, None, None, None) == H.ERR_ARG
    assert HP.api().plan(_protocol(a)._h, None, None, None, None, None) == 1  # every output may be null


def test_the_session_calls_refuse_bad_arguments_without_a_device():
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP

    a, pr = HP.api(), _protocol(PU.CircuitA(4).protocol)
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    inst = HP.pack_instances([[5]])
    out = ctypes.c_void_p(0x1234)

    def begin(p=pr._h, mos=0, tr=0, c=pc, srs=0x10000, pre=0x20000, i=inst, o=ctypes.byref(out)):
        return a.begin(p, mos, tr, c, srs, pre, i, len(inst), o)

    for name in ("p", "c", "srs", "pre", "i", "o"):
        assert begin(**{name: None}) == H.ERR_ARG, name
    assert begin(mos=2) == H.ERR_ARG and "multi-open" in HP.last_error()
    for tr in (2, 3, 7):  # the device-hashed and the routed Poseidon are the verifier's
        assert begin(tr=tr) == H.ERR_ARG and "transcript" in HP.last_error()
    assert begin(srs=0x10008) == H.ERR_ARG and begin(pre=0x20004) == H.ERR_ARG
    assert out.value is None  # *out is cleared by every call that got as far as looking at it
    n = ctypes.c_size_t(7)
    assert a.phase(None, None, 0, None, 0, ctypes.byref(n)) == H.ERR_ARG and a.finish(None, None, 0, ctypes.byref(n)) == H.ERR_ARG
    a.destroy(None)


def test_the_device_calls_refuse_bad_arguments_without_a_device():
    import snark_verifier_amd as sv

    lib = sv.load_library()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.snarkv_plonk_tail_check_dev.restype, lib.snarkv_plonk_tail_check_dev.argtypes = ctypes.c_int, [vp, vp, sz, vp]
    lib.snarkv_plonk_session_copy.restype, lib.snarkv_plonk_session_copy.argtypes = ctypes.c_int, [vp, vp, vp, sz]
    lib.snarkv_plonk_session_alloc.restype, lib.snarkv_plonk_session_alloc.argtypes = ctypes.c_int, [vp, sz, ctypes.POINTER(vp)]
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    tail, status = 0x10000, 0x90000
    check = lib.snarkv_plonk_tail_check_dev
    assert check(None, tail, 4, status) == check(pc, None, 4, status) == check(pc, tail, 4, None) == sv.SNARKV_ERR_ARG
    assert check(pc, tail + 8, 4, status) == sv.SNARKV_ERR_ARG and check(pc, tail, 4, status + 2) == sv.SNARKV_ERR_ARG
    assert check(pc, tail, (1 << 36) + 1, status) == sv.SNARKV_ERR_LENGTH
    assert check(pc, tail, 4, tail + 96) == sv.SNARKV_ERR_ARG  # the word inside the tail
    assert check(pc, tail, 0, status) == 0  # nothing to check, nothing enqueued
    copy_ = lib.snarkv_plonk_session_copy
    assert copy_(None, tail, status, 64) == copy_(pc, None, status, 64) == copy_(pc, tail, None, 64) == sv.SNARKV_ERR_ARG
    assert copy_(pc, tail, tail + 32, 64) == sv.SNARKV_ERR_ARG
    d = vp(0x1234)
    assert lib.snarkv_plonk_session_alloc(pc, 0, ctypes.byref(d)) == sv.SNARKV_ERR_EMPTY and d.value is None
    assert lib.snarkv_plonk_session_alloc(None, 64, ctypes.byref(d)) == sv.SNARKV_ERR_ARG
