"""Polynomials over the scalar field in device memory (include/snarkv_poly.h), over a BN254 `Context` or a pallas
`PallasContext`: a linear combination of many resident polynomials, the evaluation at a point and the division by a linear
factor.  Every call enqueues on the context's stream and returns; the caller synchronises before it reads a result.

Polynomials, points and results are device addresses (ints, or anything with `data_ptr()`); the indices of `lincomb` are a
list of ints and its scalars ints or 32-byte strings.

This ctypes table is this module's own, as `ipa_create`'s is: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, is_pallas, scalars as _scalars, signatures, u32s as _u32s

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_u32p = ctypes.POINTER(ctypes.c_uint32)

BLOCK = 256  # coefficients per workgroup of the scan (csrc/poly.hpp: kPolyBlock)
LINCOMB_TERMS = 32  # terms per pass of the linear combination (kPolyLincombTerms)
LAZY_TERMS = 4  # terms summed before the sum is reduced (k_poly_lincomb)

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "poly_lincomb_dev": (_int, [_vp, _vp, _sz, _sz, _u32p, _cp, _sz, _vp]),
    "poly_eval_dev": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "poly_div_linear_dev": (_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
}
# every function include/snarkv_poly.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def lincomb_dev(ctx, d_polys, n, n_polys, idx, scalars, d_out):
    """out = sum_j scalars[j] * polys[idx[j]] over a poly-major array of `n_polys` polynomials of n coefficients"""
    a = api(is_pallas(ctx))
    a.check(a.poly_lincomb_dev(ctx._h, _addr(d_polys), n, n_polys, _u32s(idx), _scalars(scalars), len(idx), _addr(d_out)))


def eval_dev(ctx, d_coeffs, n, d_point, d_out):
    """out = p(point); point and out are 32 bytes of device memory each"""
    a = api(is_pallas(ctx))
    a.check(a.poly_eval_dev(ctx._h, _addr(d_coeffs), n, _addr(d_point), _addr(d_out)))


def div_linear_dev(ctx, d_coeffs, n, d_root, d_quot, d_rem):
    """p = (X - root) quot + rem: n - 1 coefficients to d_quot (which may not overlap d_coeffs), 32 bytes to d_rem"""
    a = api(is_pallas(ctx))
    a.check(a.poly_div_linear_dev(ctx._h, _addr(d_coeffs), n, _addr(d_root), _addr(d_quot), _addr(d_rem)))
