"""The Bgh19 multi-open prover of halo2's IPA backend in one call (include/snarkv_ipa_multiopen.h), over a BN254
`Context` + `IpaDecidingKey` or a pallas `PallasContext` + `PallasIpaDecidingKey`: committed polynomials and a list of
(polynomial, shift, evaluation) queries in, the bytes `Bgh19Proof::read` consumes and the accumulator (xi, U) out.

Scalars are ints or 32-byte strings, vectors lists of ints or packed bytes, points (x, y) int pairs or 64-byte strings.
`queries` is a list of (polynomial index, shift, evaluation); the point of a query is x * shift.  `f_blind`, `p_bar` and
`omega_bar` are what the prover draws from its rng, in that order.

This ctypes table is this module's own, as `ipa_create`'s is: one table per header.
"""
import ctypes

from ._bind import bind, fe as _fe, is_pallas, prove, pt as _pt, signatures, u32s, vec as _vec

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
SIGNATURES = signatures(_SHAPES)
SIGNATURES.update(_CONTEXT_FREE)

def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, {"create_proof_default": _CONTEXT_FREE}, pallas)


def proof_bytes(k, n_sets):
    """the length of a proof over `n_sets` query sets: 64 k + 32 n_sets + 160"""
    return 64 * k + 32 * n_sets + 160


def pack_queries(queries):
    """[(poly, shift, eval)] -> the three parallel arrays of the C call: (u32 array, shifts, evaluations, count)"""
    return u32s([q[0] for q in queries]), b"".join(_fe(q[1]) for q in queries), b"".join(_fe(q[2]) for q in queries), len(queries)


def _prove(a, fn, handles, dk, h, s, polys, n_polys, blinds, x, queries, f_blind, p_bar, omega_bar, absorbed):
    """`polys` and `p_bar` as the call takes them: packed bytes or device addresses"""
    qp, qs, qe, nq = pack_queries(queries)
    cap = proof_bytes(dk.k, len(queries))  # never more sets than queries
    return prove(a, fn, dk.k, cap, *handles, _pt(h), _pt(s), polys, 1 << dk.k, n_polys, _vec(blinds), _fe(x), qp, qs, qe, nq,
                 _fe(f_blind), p_bar, _fe(omega_bar), bytes(absorbed) or None, len(absorbed))


def create_proof(ctx, dk, h, s, polys, blinds, x, queries, f_blind, p_bar, omega_bar, absorbed=b""):
    """-> (proof bytes, (xi, U)).  `polys`: a list of coefficient lists (or of packed byte strings), n = 2^k each."""
    a = api(is_pallas(ctx))
    return _prove(a, a.ipa_multiopen_create_proof, (ctx._h, dk._h), dk, h, s, b"".join(_vec(p) for p in polys) or b"\x00",
                  len(polys), blinds, x, queries, f_blind, _vec(p_bar), omega_bar, absorbed)


def create_proof_dev(ctx, dk, h, s, d_polys, n_polys, blinds, x, queries, f_blind, d_p_bar, omega_bar, absorbed=b""):
    """the same with the polynomials (n_polys x 2^k x 32 bytes, poly-major) and p_bar at device addresses"""
    a = api(is_pallas(ctx))
    return _prove(a, a.ipa_multiopen_create_proof_dev, (ctx._h, dk._h), dk, h, s, _vp(int(d_polys)), n_polys, blinds, x, queries,
                  f_blind, _vp(int(d_p_bar)), omega_bar, absorbed)


def create_proof_default(dk, h, s, polys, blinds, x, queries, f_blind, p_bar, omega_bar, absorbed=b"", pallas=False):
    """`bn254_ipa_multiopen_create_proof` / `pallas_ipa_multiopen_create_proof`: on the library's default context"""
    a = api(pallas)
    return _prove(a, a.create_proof_default, (dk._h,), dk, h, s, b"".join(_vec(p) for p in polys) or b"\x00", len(polys),
                  blinds, x, queries, f_blind, _vec(p_bar), omega_bar, absorbed)
