"""CPU: the C ABI of the PLONK prover's options (include/snarkv_host_plonk_prove_opts.h in libsnarkv_host.so): the header is
strict C99, the host library exports its two names and the device libraries do not, the second ctypes table of
snark_verifier_amd.host_plonk_prove lists exactly those names, `plan_opts` with flags = 0 is `plan`, with
SNARKV_HOST_PLONK_QUOTIENT_COSETS it reports 32 * n_cols * (N - n) bytes fewer, and the refusals that come before device work
return their codes in the plain entries' order, an unknown flag bit after them."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_host_plonk_prove_opts.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402
import plonk_prover_util as PU  # noqa: E402
import plonk_synth as S  # noqa: E402


def _protocol(pr):
    from snark_verifier_amd import host_api as H

    return H.Protocol(S.pack_protocol(pr))


def test_header_library_and_binding_agree():
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP
    from snark_verifier_amd import pallas as PL

    AU.assert_strict_c99(HDR)
    names = AU.declared(HDR, r"\b(snarkv_host_[a-z0-9_]+)\s*\(")
    assert names == sorted(HP.OPTS_SIGNATURES) == sorted(HP.PREFIX + n for n in ("plan_opts", "begin_opts"))
    assert not set(names) & (set(HP.SIGNATURES) | set(H._SIGNATURES))
    a = HP.opts_api()
    bn, pa = sv.load_library(), PL.load_library()
    for n in names:
        assert hasattr(a.lib, n) and not hasattr(bn, n) and not hasattr(pa, n), n
    assert HP.QUOTIENT_COSETS == 1


def test_plan_opts_without_a_device():
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP

    for circuit, k, n_cols in ((PU.CircuitA(4), 4, 12), (PU.CircuitB(6), 6, 17)):
        pr = _protocol(circuit.protocol)
        plain, same, cosets = HP.plan(pr), HP.plan(pr, flags=0), HP.plan(pr, flags=HP.QUOTIENT_COSETS)
        e = ctypes.c_uint32(0)
        b = ctypes.c_size_t(0)
        assert HP.opts_api().plan_opts(pr._h, 0, ctypes.byref(e), None, None, None, ctypes.byref(b)) == 1
        assert plain == same and (e.value, b.value) == (plain["e"], plain["bytes"])
        n, n_ext = 1 << k, 1 << (k + 2)
        assert plain["bytes"] == 32 * ((n_cols + 1) * n + n_cols * n_ext + n_ext)
        assert cosets["bytes"] == 32 * ((n_cols + 1) * n + n_cols * n + n_ext)  # the columns and the quotient's slot, work, h
        assert plain["bytes"] - cosets["bytes"] == 32 * n_cols * (n_ext - n)
        assert {x: v for x, v in cosets.items() if x != "bytes"} == {x: v for x, v in plain.items() if x != "bytes"}
    e0 = PU.SHAPES["e0_zero"]
    pr = _protocol(e0.protocol)
    assert HP.plan(pr)["e"] == 0 and HP.plan(pr, flags=1)["bytes"] == HP.plan(pr)["bytes"]  # e = 0: nothing to save
    a, pr = HP.opts_api(), _protocol(PU.CircuitA(4).protocol)
    assert a.plan_opts(None, 0, None, None, None, None, None) == H.ERR_ARG
    assert a.plan_opts(None, 2, None, None, None, None, None) == H.ERR_ARG and "null" in HP.last_error()
    assert a.plan_opts(pr._h, 1, None, None, None, None, None) == 1  # every output may be null
    for flags in (2, 3, 1 << 31):
        assert a.plan_opts(pr._h, flags, None, None, None, None, None) == H.ERR_ARG and "flag" in HP.last_error()
        with pytest.raises(H.HostError) as err:
            HP.plan(pr, flags=flags)
        assert err.value.code == H.ERR_ARG


def test_begin_opts_refuses_bad_arguments_without_a_device():
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP

    a, pr = HP.opts_api(), _protocol(PU.CircuitA(4).protocol)
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    inst = HP.pack_instances([[5]])
    out = ctypes.c_void_p(0x1234)

    def begin(p=pr._h, mos=0, tr=0, flags=1, c=pc, srs=0x10000, pre=0x20000, i=inst, o=ctypes.byref(out)):
        return a.begin_opts(p, mos, tr, flags, c, srs, pre, i, len(inst), o)

    for name in ("p", "c", "srs", "pre", "i", "o"):
        assert begin(**{name: None}) == H.ERR_ARG, name
    assert begin(mos=2) == H.ERR_ARG and "multi-open" in HP.last_error()
    assert begin(tr=2) == H.ERR_ARG and "transcript" in HP.last_error()
    assert begin(srs=0x10008) == H.ERR_ARG and begin(pre=0x20004) == H.ERR_ARG
    # the flag comes after the plain entry's own checks and before the context is looked at
    assert begin(flags=2) == H.ERR_ARG and "flag" in HP.last_error()
    assert begin(flags=2, mos=2) == H.ERR_ARG and "multi-open" in HP.last_error()
    assert begin(flags=6, srs=0x10008) == H.ERR_ARG and "aligned" in HP.last_error()
    assert out.value is None
