"""CPU: the C ABI of the batched evaluation, of the KZG multi-open provers and of their product call (include/snarkv_poly_batch.h,
include/snarkv_kzg_multiopen.h, include/snarkv_host_kzg_open.h): the headers are strict C99, each device library exports every declared name and only its
own (the KZG names are BN254's alone), the ctypes tables of snark_verifier_amd.poly_batch and snark_verifier_amd.kzg_multiopen
list exactly those names and share none with the tables of the other modules, and every refusal that comes before device work
returns its documented code against a fake context."""
import ctypes
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
BATCH_HDR = os.path.join(INC, "snarkv_poly_batch.h")
KZG_HDR = os.path.join(INC, "snarkv_kzg_multiopen.h")
HOST_HDR = os.path.join(INC, "snarkv_host_kzg_open.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abi_util as AU  # noqa: E402

KZG_NAMES = sorted(["snarkv_kzg_multiopen_sets", "snarkv_kzg_gwc19_create_proof", "snarkv_kzg_gwc19_create_proof_dev",
                    "snarkv_kzg_bdfg21_create_proof", "snarkv_kzg_bdfg21_create_proof_dev"])
BATCH_NAMES = sorted(["snarkv_poly_eval_many_dev", "snarkv_pallas_poly_eval_many_dev"])


def test_headers_are_strict_c99():
    for h in (BATCH_HDR, KZG_HDR, HOST_HDR):
        AU.assert_strict_c99(h)


def test_each_library_exports_its_names_and_the_tables_list_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import kzg_multiopen, poly_batch
    from snark_verifier_amd import pallas as PL

    assert AU.declared(BATCH_HDR) == BATCH_NAMES == sorted(poly_batch.SIGNATURES)
    assert AU.declared(KZG_HDR) == KZG_NAMES == sorted(kzg_multiopen.SIGNATURES)
    # no name shared with the table of any other module (abi_util.other_tables knows only the modules of its own list)
    others = set()
    for mod, attr in AU.TABLES.items():
        others |= set(getattr(importlib.import_module("snark_verifier_amd." + mod), attr))
    assert not others & set(BATCH_NAMES) and not others & set(KZG_NAMES) and not set(BATCH_NAMES) & set(KZG_NAMES)
    bn, pa = sv.load_library(), PL.load_library()
    for name in BATCH_NAMES:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for name in KZG_NAMES:
        assert hasattr(bn, name) and not hasattr(pa, name), name
        assert not hasattr(pa, name.replace("snarkv_", "snarkv_pallas_")), name
    for fn in ("gwc19_create_proof", "gwc19_create_proof_dev", "bdfg21_create_proof", "bdfg21_create_proof_dev", "n_sets"):
        assert callable(getattr(sv.kzg_multiopen, fn))
    assert callable(sv.poly_batch.eval_many_dev)


def test_eval_many_refuses_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import poly_batch as PB

    for pallas in (False, True):
        a = PB.api(pallas)
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        base, n = 0x10000, 8  # device addresses are only compared here, never followed
        points, out = base + 0x8000, base + 0x9000
        qp, qt = (ctypes.c_uint32 * 3)(0, 1, 1), (ctypes.c_uint32 * 3)(0, 0, 1)

        def call(c=pc, polys=base, n=n, npolys=2, pts=points, npts=2, qp=qp, qt=qt, count=3, o=out):
            return a.poly_eval_many_dev(c, polys, n, npolys, pts, npts, qp, qt, count, o)

        for name in ("c", "polys", "pts", "qp", "qt", "o"):
            assert call(**{name: None}) == sv.SNARKV_ERR_ARG, name
        for name, v in (("polys", base + 8), ("pts", points + 4), ("o", out + 8)):  # 16-byte alignment
            assert call(**{name: v}) == sv.SNARKV_ERR_ARG, name
        assert call(count=0) == sv.SNARKV_ERR_EMPTY and call(n=0) == sv.SNARKV_ERR_EMPTY
        assert call(npolys=0) == sv.SNARKV_ERR_EMPTY and call(npts=0) == sv.SNARKV_ERR_EMPTY
        assert call(n=(1 << 30) + 1) == sv.SNARKV_ERR_LENGTH
        assert call(qp=(ctypes.c_uint32 * 3)(0, 2, 1)) == sv.SNARKV_ERR_ARG and "index 2" in a.last_error()
        assert call(qt=(ctypes.c_uint32 * 3)(0, 0, 2)) == sv.SNARKV_ERR_ARG and "point index 2" in a.last_error()
        # out on polynomial 1, on its last coefficient, on the second point
        assert call(o=base + 32 * n) == sv.SNARKV_ERR_ARG and call(o=base + 32 * (2 * n - 1) - 64) == sv.SNARKV_ERR_ARG
        assert call(o=points + 32) == sv.SNARKV_ERR_ARG and call(o=points - 64) == sv.SNARKV_ERR_ARG
        assert "overlap" in a.last_error()


def _never(_user, _w, _out):  # the refusals below come before the first synchronisation
    raise AssertionError("draw_z_prime was called")


def test_the_provers_refuse_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import kzg_multiopen as KM

    a = KM.api()
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    n, b32 = 8, b"\x00" * 32
    one, two = (1).to_bytes(32, "little"), (2).to_bytes(32, "little")
    big = (1 << 256) - 1
    srs, polys = b"\x01" * (64 * n), b"\x00" * (32 * n * 2)
    qp = (ctypes.c_uint32 * 3)(0, 1, 1)
    ws = ctypes.create_string_buffer(b"\xaa" * 256, 256)
    count = ctypes.c_size_t(7)
    cb = KM.CHALLENGE_FN(_never)
    w, zp, wp = (ctypes.create_string_buffer(b"\xbb" * 64, 64) for _ in range(3))

    def gwc(fn=a.kzg_gwc19_create_proof, c=pc, s=srs, p=polys, n=n, npolys=2, z=one, q=qp, qs=one + one + two, qe=b32 * 3, nq=3,
            v=two, out=ws, cap=4, ns=ctypes.byref(count)):
        return fn(c, s, p, n, npolys, z, q, qs, qe, nq, v, out, cap, ns)

    def bdfg(fn=a.kzg_bdfg21_create_proof, c=pc, s=srs, p=polys, n=n, npolys=2, z=one, q=qp, qs=one + one + two, qe=b32 * 3, nq=3,
             mu=two, gamma=two, draw=cb, wo=w, zo=zp, wpo=wp):
        return fn(c, s, p, n, npolys, z, q, qs, qe, nq, mu, gamma, draw, None, wo, zo, wpo)

    for name in ("c", "s", "p", "z", "q", "qs", "qe", "v", "out", "ns"):
        assert gwc(**{name: None}) == sv.SNARKV_ERR_ARG, name
    for name in ("c", "s", "p", "z", "q", "qs", "qe", "mu", "gamma", "wo", "zo", "wpo"):
        assert bdfg(**{name: None}) == sv.SNARKV_ERR_ARG, name
    assert bdfg(draw=KM.CHALLENGE_FN(0)) == sv.SNARKV_ERR_ARG
    for call, dev in ((gwc, a.kzg_gwc19_create_proof_dev), (bdfg, a.kzg_bdfg21_create_proof_dev)):
        assert call(fn=dev, s=0x10000, p=None) == sv.SNARKV_ERR_ARG and call(fn=dev, s=None, p=0x20000) == sv.SNARKV_ERR_ARG
        assert call(fn=dev, s=0x10008, p=0x20000) == sv.SNARKV_ERR_ARG and call(fn=dev, s=0x10000, p=0x20004) == sv.SNARKV_ERR_ARG
        assert call(npolys=0) == sv.SNARKV_ERR_EMPTY and call(nq=0) == sv.SNARKV_ERR_EMPTY and call(n=0) == sv.SNARKV_ERR_EMPTY
        assert call(n=(1 << 30) + 1) == sv.SNARKV_ERR_LENGTH
        assert call(q=(ctypes.c_uint32 * 3)(0, 2, 1)) == sv.SNARKV_ERR_ARG and "polynomial 2 of 2" in a.last_error()
    # ws_cap one short: two sets (shift 1, shift 2); the needed count comes back, nothing else is written
    assert gwc(cap=1) == sv.SNARKV_ERR_LENGTH and count.value == 2
    assert gwc(cap=0, nq=2) == sv.SNARKV_ERR_LENGTH and count.value == 1
    # Bdfg21: polynomial 1 is queried at two shifts.  z = 0 puts both points at 0; n = 1 is fewer coefficients than points
    assert bdfg(z=b32) == sv.SNARKV_ERR_ARG and "coincide" in a.last_error()
    assert bdfg(n=1) == sv.SNARKV_ERR_ARG and "more points" in a.last_error()
    # SNARKV_FLAG_VALIDATE is a default flag of the context (csrc/ctx.hpp: `flags` lies behind the slots and the host buffers)
    strict = AU.FakeCtx(device=0)
    ctypes.memset(ctypes.addressof(strict) + 4, 0xFF, 8192)  # every flag set, whatever the field's offset
    ps = ctypes.addressof(strict)
    bad = big.to_bytes(32, "little")
    for call in (gwc, bdfg):
        assert call(c=ps, z=bad) == sv.SNARKV_ERR_ENCODING
        assert call(c=ps, qs=one + bad + two) == sv.SNARKV_ERR_ENCODING and call(c=ps, qe=b32 * 2 + bad) == sv.SNARKV_ERR_ENCODING
    assert gwc(c=ps, v=bad) == sv.SNARKV_ERR_ENCODING
    assert bdfg(c=ps, mu=bad) == sv.SNARKV_ERR_ENCODING and bdfg(c=ps, gamma=bad) == sv.SNARKV_ERR_ENCODING
    assert ws.raw == b"\xaa" * 256 and w.raw == zp.raw == wp.raw == b"\xbb" * 64


def test_the_product_call_is_exported_bound_and_refuses_bad_arguments_without_a_device():
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_kzg_open as HK
    from snark_verifier_amd import pallas as PL

    names = AU.declared(HOST_HDR, r"\b(snarkv_host_[a-z0-9_]+)\s*\(")
    assert names == ["snarkv_host_kzg_open"] == sorted(HK.SIGNATURES)
    assert not set(names) & set(H._SIGNATURES)
    lib = HK.api()
    assert not hasattr(sv.load_library(), names[0]) and not hasattr(PL.load_library(), names[0])
    ctx = AU.FakeCtx(device=0)
    pc = ctypes.addressof(ctx)
    one, big = (1).to_bytes(32, "little"), b"\xff" * 32
    qp = (ctypes.c_uint32 * 2)(0, 0)
    proof, plen, ch = ctypes.create_string_buffer(b"\xaa" * 256, 256), ctypes.c_size_t(9), ctypes.create_string_buffer(96)

    def call(mos=0, tr=0, c=pc, s=0x10000, p=0x20000, n=8, npolys=1, z=one, q=qp, qs=one * 2, qe=one * 2, nq=2, pre=None, prelen=0,
             out=proof, cap=256, ln=ctypes.byref(plen)):
        return lib.snarkv_host_kzg_open(mos, tr, c, s, p, n, npolys, z, q, qs, qe, nq, pre, prelen, out, cap, ln, ch)

    for name in ("c", "s", "p", "z", "q", "qs", "qe", "ln"):
        assert call(**{name: None}) == H.ERR_ARG, name
    assert call(prelen=3) == H.ERR_ARG  # prefix bytes announced, none given
    assert call(mos=2) == H.ERR_ARG and b"multi-open" in lib.snarkv_host_last_error()
    assert call(tr=7) == H.ERR_ARG and b"transcript" in lib.snarkv_host_last_error()
    assert call(z=big) == H.ERR_ARG and call(qs=one + big) == H.ERR_ARG and call(qe=big + one) == H.ERR_ARG
    assert call(pre=b"\x03", prelen=1) == H.ERR_ARG and call(pre=b"\x00" + one[:20], prelen=21) == H.ERR_ARG  # unknown tag, short item
    assert call(pre=b"\x00" + big, prelen=33) == H.ERR_ARG
    assert plen.value == 0 and proof.raw == b"\xaa" * 256
    assert HK.pack_prefix([("scalar", 5), ("squeeze",), ("point", b"\x01" * 64)]) == b"\x00" + (5).to_bytes(32, "little") + b"\x02\x01" + b"\x01" * 64
