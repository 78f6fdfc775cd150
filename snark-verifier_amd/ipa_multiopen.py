"""The Bgh19 multi-open prover of halo2's IPA backend in one call (include/snarkv_ipa_multiopen.h), over a BN254
`Context` + `IpaDecidingKey` or a pallas `PallasContext` + `PallasIpaDecidingKey`: committed polynomials and a list of
(polynomial, shift, evaluation) queries in, the bytes `Bgh19Proof::read` consumes and the accumulator (xi, U) out.

Scalars are ints or 32-byte strings, vectors lists of ints or packed bytes, points (x, y) int pairs or 64-byte strings.
`queries` is a list of (polynomial index, shift, evaluation); the point of a query is x * shift.  `f_blind`, `p_bar` and
`omega_bar` are what the prover draws from its rng, in that order.

This ctypes table is this module's own, as `ipa_create`'s is: one table per header.
"""
import ctypes

from ._lib import SnarkvError
from .ipa_create import _fe, _pt, _vec

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_szp = ctypes.POINTER(ctypes.c_size_t)
_u32p = ctypes.POINTER(ctypes.c_uint32)

_QUERIES = [_cp, _cp, _u32p, _cp, _cp, _sz, _cp]  # blinds, x, q_poly, q_shift, q_eval, n_queries, f_blind
_TAIL = [_cp, _cp, _sz, _vp, _sz, _szp, _vp, _vp]  # omega_bar, absorbed, its length, proof_out, proof_cap, proof_len, xi_out, u_out
# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_multiopen_create_proof": (_int, [_vp, _vp, _cp, _cp, _cp, _sz, _sz] + _QUERIES + [_cp] + _TAIL),
    "ipa_multiopen_create_proof_dev": (_int, [_vp, _vp, _cp, _cp, _vp, _sz, _sz] + _QUERIES + [_vp] + _TAIL),
}
# the forms on a library's default context
_CONTEXT_FREE = {
    "bn254_ipa_multiopen_create_proof": (_int, [_vp, _cp, _cp, _cp, _sz, _sz] + _QUERIES + [_cp] + _TAIL),
    "pallas_ipa_multiopen_create_proof": (_int, [_vp, _cp, _cp, _cp, _sz, _sz] + _QUERIES + [_cp] + _TAIL),
}
# every function include/snarkv_ipa_multiopen.h declares
SIGNATURES = {p + n: s for p in ("snarkv_", "snarkv_pallas_") for n, s in _SHAPES.items()}
SIGNATURES.update(_CONTEXT_FREE)

_BOUND = {}


class _Api:
    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        free = ("pallas" if prefix == "snarkv_pallas_" else "bn254") + "_ipa_multiopen_create_proof"
        for name, (res, args) in [(prefix + n, s) for n, s in _SHAPES.items()] + [(free, _CONTEXT_FREE[free])]:
            fn = getattr(lib, name)  # AttributeError if the header and the library drift
            fn.restype, fn.argtypes = res, args
        self.create_proof_default = getattr(lib, free)

    def __getattr__(self, name):
        return getattr(self.lib, self.prefix + name)

    def last_error(self):
        err = self.lib.snarkv_pallas_last_error if self.prefix == "snarkv_pallas_" else self.lib.snarkv_last_error
        return (err() or b"").decode(errors="replace")

    def check(self, rc):
        if rc < 0:
            raise SnarkvError(rc, self.last_error())
        return rc


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    if pallas not in _BOUND:
        if pallas:
            from .pallas import load_library

            _BOUND[pallas] = _Api(load_library(), "snarkv_pallas_")
        else:
            from ._lib import load_library

            _BOUND[pallas] = _Api(load_library(), "snarkv_")
    return _BOUND[pallas]


def _is_pallas(ctx):
    from .pallas import PallasContext

    return isinstance(ctx, PallasContext)


def proof_bytes(k, n_sets):
    """the length of a proof over `n_sets` query sets: 64 k + 32 n_sets + 160"""
    return 64 * k + 32 * n_sets + 160


def pack_queries(queries):
    """[(poly, shift, eval)] -> the three parallel arrays of the C call: (u32 array, shifts, evaluations, count)"""
    polys = (ctypes.c_uint32 * max(len(queries), 1))(*[q[0] for q in queries])
    return polys, b"".join(_fe(q[1]) for q in queries), b"".join(_fe(q[2]) for q in queries), len(queries)


def _outs(k, queries):
    cap = proof_bytes(k, len(queries))  # never more sets than queries
    return ctypes.create_string_buffer(cap), cap, ctypes.c_size_t(0), ctypes.create_string_buffer(32 * max(k, 1)), \
        ctypes.create_string_buffer(64)


def _finish(a, k, rc, proof, plen, xi, u):
    a.check(rc)
    xis = [int.from_bytes(xi.raw[32 * i:32 * i + 32], "little") for i in range(k)]
    x, y = int.from_bytes(u.raw[:32], "little"), int.from_bytes(u.raw[32:], "little")
    return proof.raw[:plen.value], (xis, (x, y))


def create_proof(ctx, dk, h, s, polys, blinds, x, queries, f_blind, p_bar, omega_bar, absorbed=b""):
    """-> (proof bytes, (xi, U)).  `polys`: a list of coefficient lists (or of packed byte strings), n = 2^k each."""
    a = api(_is_pallas(ctx))
    pb = b"".join(_vec(p) for p in polys)
    n = 1 << dk.k
    qp, qs, qe, nq = pack_queries(queries)
    proof, cap, plen, xi, u = _outs(dk.k, queries)
    rc = a.ipa_multiopen_create_proof(ctx._h, dk._h, _pt(h), _pt(s), pb or b"\x00", n, len(polys), _vec(blinds) or b"\x00", _fe(x),
                                      qp, qs or b"\x00", qe or b"\x00", nq, _fe(f_blind), _vec(p_bar), _fe(omega_bar),
                                      bytes(absorbed) or None, len(absorbed), proof, cap, ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)


def create_proof_dev(ctx, dk, h, s, d_polys, n_polys, blinds, x, queries, f_blind, d_p_bar, omega_bar, absorbed=b""):
    """the same with the polynomials (n_polys x 2^k x 32 bytes, poly-major) and p_bar at device addresses"""
    a = api(_is_pallas(ctx))
    qp, qs, qe, nq = pack_queries(queries)
    proof, cap, plen, xi, u = _outs(dk.k, queries)
    rc = a.ipa_multiopen_create_proof_dev(ctx._h, dk._h, _pt(h), _pt(s), _vp(int(d_polys)), 1 << dk.k, n_polys, _vec(blinds), _fe(x),
                                          qp, qs, qe, nq, _fe(f_blind), _vp(int(d_p_bar)), _fe(omega_bar),
                                          bytes(absorbed) or None, len(absorbed), proof, cap, ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)


def create_proof_default(dk, h, s, polys, blinds, x, queries, f_blind, p_bar, omega_bar, absorbed=b"", pallas=False):
    """`bn254_ipa_multiopen_create_proof` / `pallas_ipa_multiopen_create_proof`: on the library's default context"""
    a = api(pallas)
    pb = b"".join(_vec(p) for p in polys)
    qp, qs, qe, nq = pack_queries(queries)
    proof, cap, plen, xi, u = _outs(dk.k, queries)
    rc = a.create_proof_default(dk._h, _pt(h), _pt(s), pb or b"\x00", 1 << dk.k, len(polys), _vec(blinds) or b"\x00", _fe(x), qp,
                                qs or b"\x00", qe or b"\x00", nq, _fe(f_blind), _vec(p_bar), _fe(omega_bar),
                                bytes(absorbed) or None, len(absorbed), proof, cap, ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)
