"""Many evaluations of resident polynomials in one call (include/snarkv_poly_batch.h), over a BN254 `Context` or a pallas
`PallasContext`: out[i] = polys[q_poly[i]](points[q_point[i]]).  The call enqueues on the context's stream and returns; the
caller synchronises before it reads a result.  The number of launches depends on n, not on the number of queries.

Polynomials, points and results are device addresses (ints, or anything with `data_ptr()`); the two index lists are lists of
ints.

This ctypes table is this module's own, as `poly`'s is: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, is_pallas, signatures, u32s as _u32s

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
_u32p = ctypes.POINTER(ctypes.c_uint32)

GRID_QUERIES = 65535  # queries per launch (csrc/poly_batch.hip: kBatchGridY)

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "poly_eval_many_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _u32p, _u32p, _sz, _vp]),
}
# every function include/snarkv_poly_batch.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def eval_many_dev(ctx, d_polys, n, n_polys, d_points, n_points, q_poly, q_point, d_out):
    """out[i] = polys[q_poly[i]](points[q_point[i]]) over a poly-major array of `n_polys` polynomials of n coefficients and
    `n_points` points of 32 bytes; `d_out` takes len(q_poly) results of 32 bytes"""
    if len(q_poly) != len(q_point):
        raise ValueError("eval_many_dev: one point index per polynomial index")
    a = api(is_pallas(ctx))
    a.check(a.poly_eval_many_dev(ctx._h, _addr(d_polys), n, n_polys, _addr(d_points), n_points, _u32s(q_poly), _u32s(q_point),
                                 len(q_poly), _addr(d_out)))
