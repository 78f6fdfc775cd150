"""CPU: the C ABI of the PLONK prover on pallas (include/snarkv_host_pallas_plonk_prove.h in
libsnarkv_host_pallas_plonk_prove.so, and the device side it adds, include/snarkv_pallas_session.h in libsnarkv_pallas.so): the
headers are strict C99, each library exports the names of its header and no other library does, the ctypes table of
snark_verifier_amd.host_plonk_prove_pallas lists exactly the host header's names, `plan` gives the compiled plan's numbers
without a device and refuses what the prover refuses, and every refusal that comes before device work returns its documented
code."""
import copy
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HOST_HDR = os.path.join(INC, "snarkv_host_pallas_plonk_prove.h")
DEV_HDR = os.path.join(INC, "snarkv_pallas_session.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402
import pallas as PA  # noqa: E402
import plonk_prover_pallas_util as PP  # noqa: E402
import plonk_synth as S  # noqa: E402

DEV_NAMES = sorted("snarkv_pallas_" + n for n in ("session_alloc", "session_free", "session_upload", "session_copy",
                                                  "session_download", "poly_tail_check_dev"))
HOST_NAMES = sorted("snarkv_host_pallas_plonk_prover_" + n for n in ("plan", "begin", "phase", "finish", "destroy", "last_error"))


def _exported(lib):
    r = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {f[-1] for f in (line.split() for line in r.stdout.splitlines()) if f}


def test_headers_are_strict_c99():
    for h in (HOST_HDR, DEV_HDR):
        AU.assert_strict_c99(h)


def test_header_library_and_binding_agree():
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_api_pallas as HA
    from snark_verifier_amd import host_plonk_prove as HK
    from snark_verifier_amd import host_plonk_prove_pallas as HP
    from snark_verifier_amd import pallas as PL

    assert AU.declared(HOST_HDR, r"\b(snarkv_host_[a-z0-9_]+)\s*\(") == sorted(HP.SIGNATURES) == HOST_NAMES
    taken = set(H._SIGNATURES) | set(HK.SIGNATURES) | set(HK.OPTS_SIGNATURES) | set(HA._SIGNATURES) | set(HA._FOLD_SIGNATURES) | \
        set(HA._PROVE_SIGNATURES)
    assert not set(HOST_NAMES) & taken
    a = HP.api()
    assert sorted(s for s in _exported(a.lib) if s.startswith("snarkv_")) == HOST_NAMES  # exactly its header's names
    bn, pa = sv.load_library(), PL.load_library()
    others = [bn, pa, H.load_library(), HA.load_library(), HA.load_fold_library(), HA.load_prove_library()]
    for n in HOST_NAMES:
        assert hasattr(a.lib, n) and not any(hasattr(o, n) for o in others), n
        fn = getattr(a.lib, n)  # what `a.<name>` resolves to (`a.last_error` is the binder's decoded form of it)
        assert (fn.restype, fn.argtypes) == HP.SIGNATURES[n]
    # the device side: its six names in libsnarkv_pallas.so alone, in no binding table, and nothing under the BN254 spelling
    assert AU.declared(DEV_HDR) == DEV_NAMES
    tables = set()
    for mod, attr in AU.TABLES.items():
        tables |= set(getattr(__import__("snark_verifier_amd." + mod, fromlist=[attr]), attr))
    assert not tables & set(DEV_NAMES)
    pa_exports = _exported(pa)
    for n in DEV_NAMES:
        assert n in pa_exports and not hasattr(bn, n) and not hasattr(bn, n.replace("snarkv_pallas_", "snarkv_")), n
    assert callable(sv.host_plonk_prove_pallas.plan) and callable(sv.host_plonk_prove_pallas.PlonkProver)


def _protocol(pr):
    from snark_verifier_amd import host_api_pallas as HA

    with PP.on_pallas():
        return HA.Protocol(S.pack_protocol(pr))


def test_plan_without_a_device():
    from snark_verifier_amd import host_api_pallas as HA
    from snark_verifier_amd import host_plonk_prove_pallas as HP

    for circuit, k, n_cols in ((PP.CircuitA(4), 4, 12), (PP.CircuitB(4), 4, 17)):
        n, n_ext = 1 << k, 1 << (k + 2)
        for flags, work in ((0, n_ext), (HP.QUOTIENT_COSETS, n)):
            p = HP.plan(_protocol(circuit.protocol), flags)
            assert (p["e"], p["n_cols"]) == (2, n_cols) and 0 < p["n_instr"] <= 4096 and 0 < p["n_consts"] <= 1024
            assert p["bytes"] == 32 * ((n_cols + 1) * n + n_cols * work + n_ext)  # the columns and the quotient's slot, work, h
    a = PP.CircuitA(4).protocol
    with PP.on_pallas():
        far = PP.P.Domain(29)
    ick = {"bases": [PA.G1_GEN], "constant": None}
    for change, word in (({"linearization": "WithoutConstant"}, "linearization"),
                         ({"instance_committing_key": ick}, "instance_committing_key"),
                         ({"queries": a["queries"] + [(5, 0)]}, "instance polynomial"),
                         ({"quotient": dict(a["quotient"], chunk_degree=2)}, "chunk_degree"),
                         ({"quotient": dict(a["quotient"], numerator=("lagrange", 600))}, "Lagrange"),
                         ({"quotient": dict(a["quotient"], num_chunk=5)}, "num_chunk"),
                         ({"domain": far}, "k + e")):
        pr = copy.copy(a)
        pr.update(change)
        with pytest.raises(HA.HostError) as e:
            HP.plan(_protocol(pr))
        assert e.value.code == HA.ERR_INVALID_PROTOCOL and word in str(e.value), change
    assert HP.api().plan(None, 0, None, None, None, None, None) == HA.ERR_ARG
    assert HP.api().plan(_protocol(a)._h, 2, None, None, None, None, None) == HA.ERR_ARG and "flag" in HP.last_error()
    assert HP.api().plan(_protocol(a)._h, 0, None, None, None, None, None) == 1  # every output may be null


def test_the_session_calls_refuse_bad_arguments_without_a_device():
    from snark_verifier_amd import host_api_pallas as HA
    from snark_verifier_amd import host_plonk_prove_pallas as HP

    a, pr = HP.api(), _protocol(PP.CircuitA(4).protocol)
    ctx, key = AU.FakeCtx(device=0), AU.FakeKey(device=0, k=4, d_points=0x40000, first=0, count=16)
    pc, pk = ctypes.addressof(ctx), ctypes.addressof(key)
    inst = HP.pack_instances([[5]])
    pt, blinds = bytes(range(64)), bytes(32 * 5)
    out = ctypes.c_void_p(0x1234)

    def begin(p=pr._h, flags=0, c=pc, dk=pk, h=pt, s=pt, pre=0x20000, pb=blinds, i=inst, o=ctypes.byref(out)):
        return a.begin(p, flags, c, dk, h, s, pre, pb, i, len(inst), o)

    for name in ("p", "c", "dk", "h", "s", "pre", "pb", "i", "o"):
        assert begin(**{name: None}) == HA.ERR_ARG, name
    assert begin(h=None) == HA.ERR_ARG and "zero-knowledge" in HP.last_error()
    assert begin(flags=2) == HA.ERR_ARG and "flag" in HP.last_error()
    assert begin(pre=0x20004) == HA.ERR_ARG and "aligned" in HP.last_error()
    for k in (3, 5):  # a key of another size
        other = AU.FakeKey(device=0, k=k, d_points=0x40000, first=0, count=1 << k)
        assert begin(dk=ctypes.addressof(other)) == HA.ERR_ARG and "2^k" in HP.last_error()
    assert out.value is None  # *out is cleared by every call that got as far as looking at it
    n = ctypes.c_size_t(7)
    assert a.phase(None, None, 0, None, None, 0, ctypes.byref(n)) == HA.ERR_ARG
    assert a.finish(None, None, None, None, None, None, 0, ctypes.byref(n), None) == HA.ERR_ARG
    a.destroy(None)


def test_the_device_calls_refuse_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    lib = PL.load_library()
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    for name, res, args in (("session_alloc", i, [vp, sz, ctypes.POINTER(vp)]), ("session_free", None, [vp, vp]),
                            ("session_upload", i, [vp, vp, vp, sz]), ("session_copy", i, [vp, vp, vp, sz]),
                            ("session_download", i, [vp, vp, vp, sz]), ("poly_tail_check_dev", i, [vp, vp, sz, vp])):
        fn = getattr(lib, "snarkv_pallas_" + name)
        fn.restype, fn.argtypes = res, args
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    host = ctypes.create_string_buffer(64)
    tail, status = 0x10000, 0x90000
    check = lib.snarkv_pallas_poly_tail_check_dev
    assert check(None, tail, 4, status) == check(pc, None, 4, status) == check(pc, tail, 4, None) == sv.SNARKV_ERR_ARG
    assert check(pc, tail + 8, 4, status) == sv.SNARKV_ERR_ARG and check(pc, tail, 4, status + 2) == sv.SNARKV_ERR_ARG
    assert check(pc, tail, (1 << 36) + 1, status) == sv.SNARKV_ERR_LENGTH
    assert check(pc, tail, 4, tail + 96) == sv.SNARKV_ERR_ARG  # the word inside the tail
    assert check(pc, tail, 0, status) == 0  # nothing to check, nothing enqueued
    copy_ = lib.snarkv_pallas_session_copy
    assert copy_(None, tail, status, 64) == copy_(pc, None, status, 64) == copy_(pc, tail, None, 64) == sv.SNARKV_ERR_ARG
    assert copy_(pc, tail, tail + 32, 64) == sv.SNARKV_ERR_ARG and copy_(pc, tail, status, 0) == 0
    up, down = lib.snarkv_pallas_session_upload, lib.snarkv_pallas_session_download
    assert up(None, tail, host, 64) == up(pc, None, host, 64) == up(pc, tail, None, 64) == sv.SNARKV_ERR_ARG and up(pc, tail, host, 0) == 0
    assert down(None, host, tail, 64) == down(pc, None, tail, 64) == down(pc, host, None, 64) == sv.SNARKV_ERR_ARG
    d = vp(0x1234)
    assert lib.snarkv_pallas_session_alloc(pc, 0, ctypes.byref(d)) == sv.SNARKV_ERR_EMPTY and d.value is None
    assert lib.snarkv_pallas_session_alloc(None, 64, ctypes.byref(d)) == sv.SNARKV_ERR_ARG
    assert lib.snarkv_pallas_session_alloc(pc, 64, None) == sv.SNARKV_ERR_ARG
    lib.snarkv_pallas_session_free(None, tail)  # ignored, as a null address is
    lib.snarkv_pallas_session_free(pc, None)
