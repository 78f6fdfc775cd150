"""The provers of the two KZG multi-open schemes on BN254 (include/snarkv_kzg_multiopen.h), over a `Context`: committed
polynomials and a list of (polynomial, shift, evaluation) queries in, the opening points `Gwc19Proof::read` /
`Bdfg21Proof::read` consume out.  The caller owns the challenges; Bdfg21's z' is drawn by a callback that is handed W.

Scalars are ints or 32-byte strings, points come back as 64-byte strings (x || y, the identity as 64 zero bytes).  `queries`
is a list of (polynomial index, shift, evaluation); the point of a query is z * shift.

This ctypes table is this module's own: one table per header.  The names exist in libsnarkv_amd.so only.
"""
import ctypes

from ._bind import addr as _addr, bind, fe as _fe, vec as _vec
from .ipa_multiopen import pack_queries

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_szp = ctypes.POINTER(ctypes.c_size_t)
_u32p = ctypes.POINTER(ctypes.c_uint32)

MOS_GWC19, MOS_BDFG21 = 0, 1  # SNARKV_KZG_MOS_*, the values of SNARKV_HOST_MOS_*

# int (*)(void* user, const uint8_t w64[64], uint8_t z_prime32[32])
CHALLENGE_FN = ctypes.CFUNCTYPE(_int, _vp, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8))

_QUERIES = [_cp, _u32p, _cp, _cp, _sz]  # z, q_poly, q_shift, q_eval, n_queries
_GWC_TAIL = [_cp, _vp, _sz, _szp]  # v, ws_out, ws_cap, n_sets_out
_BDFG_TAIL = [_cp, _cp, CHALLENGE_FN, _vp, _vp, _vp, _vp]  # mu, gamma, draw_z_prime, user, w_out, z_prime_out, w_prime_out
# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "kzg_multiopen_sets": (_int, [_int, _u32p, _cp, _sz, _szp]),
    "kzg_gwc19_create_proof": (_int, [_vp, _cp, _cp, _sz, _sz] + _QUERIES + _GWC_TAIL),
    "kzg_gwc19_create_proof_dev": (_int, [_vp, _vp, _vp, _sz, _sz] + _QUERIES + _GWC_TAIL),
    "kzg_bdfg21_create_proof": (_int, [_vp, _cp, _cp, _sz, _sz] + _QUERIES + _BDFG_TAIL),
    "kzg_bdfg21_create_proof_dev": (_int, [_vp, _vp, _vp, _sz, _sz] + _QUERIES + _BDFG_TAIL),
}
# every function include/snarkv_kzg_multiopen.h declares
SIGNATURES = {"snarkv_" + n: s for n, s in _SHAPES.items()}


def api():
    """the functions in libsnarkv_amd.so"""
    return bind(_SHAPES, None, False)


def n_sets(mos, queries):
    """the number of query sets of a query list under `mos` (MOS_GWC19 / MOS_BDFG21)"""
    a = api()
    qp, qs, _, nq = pack_queries([(q[0], q[1], 0) for q in queries])
    out = ctypes.c_size_t(0)
    a.check(a.kzg_multiopen_sets(mos, qp, qs, nq, ctypes.byref(out)))
    return out.value


def _gwc19(a, fn, ctx, srs, polys, n, n_polys, z, queries, v):
    qp, qs, qe, nq = pack_queries(queries)
    ws, count = ctypes.create_string_buffer(64 * max(nq, 1)), ctypes.c_size_t(0)  # never more sets than queries
    a.check(fn(ctx._h, srs, polys, n, n_polys, _fe(z), qp, qs, qe, nq, _fe(v), ws, nq, ctypes.byref(count)))
    return [ws.raw[64 * i:64 * i + 64] for i in range(count.value)]


def gwc19_create_proof(ctx, srs, polys, z, queries, v):
    """-> [W_1, .., W_S].  `srs`: n points packed (64 bytes each); `polys`: a list of coefficient lists (or of packed byte
    strings), n coefficients each"""
    a = api()
    packed = b"".join(_vec(p) for p in polys) or b"\x00"
    return _gwc19(a, a.kzg_gwc19_create_proof, ctx, bytes(srs), packed, len(srs) // 64, len(polys), z, queries, v)


def gwc19_create_proof_dev(ctx, d_srs, d_polys, n, n_polys, z, queries, v):
    """the same with the SRS (n x 64 bytes) and the polynomials (n_polys x n x 32 bytes, poly-major) at device addresses"""
    a = api()
    return _gwc19(a, a.kzg_gwc19_create_proof_dev, ctx, _addr(d_srs), _addr(d_polys), n, n_polys, z, queries, v)


def _bdfg21(a, fn, ctx, srs, polys, n, n_polys, z, queries, mu, gamma, draw_z_prime):
    qp, qs, qe, nq = pack_queries(queries)
    w, zp, wp = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    raised = []

    def cb(_user, w64, out32):
        try:
            zprime = draw_z_prime(bytes(w64[:64]))
            if zprime is None:
                return 1
            ctypes.memmove(out32, _fe(zprime), 32)
            return 0
        except Exception as e:  # an exception must not cross the C frames: the call ends with SNARKV_ERR_ARG
            raised.append(e)
            return 1

    rc = fn(ctx._h, srs, polys, n, n_polys, _fe(z), qp, qs, qe, nq, _fe(mu), _fe(gamma), CHALLENGE_FN(cb), None, w, zp, wp)
    if raised:
        raise raised[0]
    a.check(rc)
    return w.raw, int.from_bytes(zp.raw, "little"), wp.raw


def bdfg21_create_proof(ctx, srs, polys, z, queries, mu, gamma, draw_z_prime):
    """-> (W, z', W').  `draw_z_prime(W bytes)` returns z' (an int or 32 bytes; None fails the call) and runs on the calling
    thread between the call's two synchronisations; it must not use `ctx`"""
    a = api()
    packed = b"".join(_vec(p) for p in polys) or b"\x00"
    return _bdfg21(a, a.kzg_bdfg21_create_proof, ctx, bytes(srs), packed, len(srs) // 64, len(polys), z, queries, mu, gamma,
                   draw_z_prime)


def bdfg21_create_proof_dev(ctx, d_srs, d_polys, n, n_polys, z, queries, mu, gamma, draw_z_prime):
    """the same with the SRS and the polynomials at device addresses"""
    a = api()
    return _bdfg21(a, a.kzg_bdfg21_create_proof_dev, ctx, _addr(d_srs), _addr(d_polys), n, n_polys, z, queries, mu, gamma,
                   draw_z_prime)
