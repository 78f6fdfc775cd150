"""The prover's half of the two KZG multi-open schemes through the product API of the host mirror
(include/snarkv_host_kzg_open.h, libsnarkv_host.so): `Gwc19::create_proof` / `Bdfg21::create_proof` over a fresh EVM or
Poseidon transcript to which a prefix is replayed first, on resident polynomials of a `Context`.

`prefix` is a list of items: ("scalar", int or 32 bytes), ("point", 64 bytes) -- both written -- and ("squeeze",) -- a
challenge squeezed and discarded.  `queries` is a list of (polynomial index, shift, evaluation).

This ctypes table is this module's own: one table per header."""
import ctypes

from . import host_api as H
from ._bind import addr as _addr, fe as _fe
from .ipa_multiopen import pack_queries

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_u32p = ctypes.POINTER(ctypes.c_uint32)

MOS_GWC19, MOS_BDFG21 = 0, 1
TRANSCRIPT_EVM, TRANSCRIPT_POSEIDON = 0, 1

# every function include/snarkv_host_kzg_open.h declares
SIGNATURES = {
    "snarkv_host_kzg_open": (_int, [_int, _int, _vp, _vp, _vp, _sz, _sz, _cp, _u32p, _cp, _cp, _sz, _cp, _sz, _vp, _sz,
                                    ctypes.POINTER(_sz), _vp]),
}
_bound = None


def api():
    global _bound
    if _bound is None:
        lib = H.load_library()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the header and the library drift
            fn.restype, fn.argtypes = res, args
        _bound = lib
    return _bound


def pack_prefix(items):
    out = b""
    for it in items:
        if it[0] == "scalar":
            out += b"\x00" + _fe(it[1])
        elif it[0] == "point":
            out += b"\x01" + bytes(it[1])
        elif it[0] == "squeeze":
            out += b"\x02"
        else:
            raise ValueError("prefix item %r" % (it,))
    return out


def kzg_open(mos, transcript, ctx, d_srs, d_polys, n, n_polys, z, queries, prefix=()):
    """-> (verdict, the bytes the opening wrote, the challenges: [v] or [mu, gamma, z']).  verdict 1: written; 0: the
    mirror's assertion failure (an evaluation that does not match); a negative code raises `HostError`"""
    lib = api()
    qp, qs, qe, nq = pack_queries(queries)
    pre = pack_prefix(prefix)
    proof, plen = ctypes.create_string_buffer(64 * max(nq, 2)), ctypes.c_size_t(0)
    ch = ctypes.create_string_buffer(96)
    rc = lib.snarkv_host_kzg_open(mos, transcript, ctx._h, _addr(d_srs), _addr(d_polys), n, n_polys, _fe(z), qp, qs, qe, nq, pre or None,
                                  len(pre), proof, len(proof), ctypes.byref(plen), ch)
    if rc < 0:
        raise H.HostError(rc, (lib.snarkv_host_last_error() or b"").decode(errors="replace"))
    count = 1 if mos == MOS_GWC19 else 3
    return rc, proof.raw[:plen.value], [int.from_bytes(ch.raw[32 * i:32 * i + 32], "little") for i in range(count)]
