"""Products along columns of scalars in device memory (include/snarkv_poly_prod.h), over a BN254 `Context` or a pallas
`PallasContext`: the pointwise product (`mul_dev`), the product of affine terms (`prod_affine_dev`), the batch inversion
(`batch_invert_dev`), the grand product (`grand_product_dev`) and the permutation argument's column Z (`perm_product_dev`).
Every call enqueues on the context's stream and returns; the caller synchronises before it reads a result.

Columns, start values and totals are device addresses (ints, or anything with `data_ptr()`); indices are lists of ints
(`NONE`: a term without a beta part) and scalars ints or 32-byte strings.

This ctypes table is this module's own, as `poly`'s and `ntt`'s are: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, fe as _fe, is_pallas, scalars as _scalars, signatures, u32s as _idx

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_u32p = ctypes.POINTER(ctypes.c_uint32)

NONE = 0xFFFFFFFF  # SNARKV_POLY_NONE
BLOCK = 1024  # elements per workgroup at level 0 of the scans (csrc/poly_prod.hip: kProdBlock)
LEVEL_BLOCK = 256  # ... at the levels above (kProdLevelBlock)
AFFINE_TERMS = 16  # terms per pass of the affine product (kProdAffineTerms)

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "poly_mul_dev": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "poly_prod_affine_dev": (_int, [_vp, _vp, _sz, _sz, _u32p, _u32p, _cp, _cp, _sz, _vp]),
    "poly_batch_invert_dev": (_int, [_vp, _vp, _sz, _vp]),
    "poly_grand_product_dev": (_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "poly_perm_product_dev": (_int, [_vp, _vp, _sz, _sz, _u32p, _u32p, _u32p, _sz, _cp, _cp, _vp, _vp, _vp, _vp]),
}
# every function include/snarkv_poly_prod.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def mul_dev(ctx, d_a, d_b, n, d_out):
    """out[i] = a[i] * b[i]; out may be a or b"""
    a = api(is_pallas(ctx))
    a.check(a.poly_mul_dev(ctx._h, _addr(d_a), _addr(d_b), n, _addr(d_out)))


def prod_affine_dev(ctx, d_polys, n, n_polys, idx_a, idx_b, betas, gammas, d_out):
    """out[i] = prod_j (polys[idx_a[j]][i] + betas[j] * polys[idx_b[j]][i] + gammas[j]); idx_b[j] = NONE: no beta part"""
    a = api(is_pallas(ctx))
    assert len(idx_a) == len(idx_b) == len(betas) == len(gammas)
    a.check(a.poly_prod_affine_dev(ctx._h, _addr(d_polys), n, n_polys, _idx(idx_a), _idx(idx_b), _scalars(betas),
                                   _scalars(gammas), len(idx_a), _addr(d_out)))


def batch_invert_dev(ctx, d_in, n, d_out):
    """out[i] = 1 / in[i], and 0 where in[i] is zero; out may be in"""
    a = api(is_pallas(ctx))
    a.check(a.poly_batch_invert_dev(ctx._h, _addr(d_in), n, _addr(d_out)))


def grand_product_dev(ctx, d_f, n, d_out, d_start=None, d_total=None):
    """out[0] = start (1 without one), out[i] = out[i-1] * f[i-1]; total = out[n-1] * f[n-1]; out may be f"""
    a = api(is_pallas(ctx))
    a.check(a.poly_grand_product_dev(ctx._h, _addr(d_f), n, _addr(d_start), _addr(d_out), _addr(d_total)))


def perm_product_dev(ctx, d_polys, n, n_polys, idx_v, idx_id, idx_sigma, beta, gamma, d_work, d_z, d_start=None, d_total=None):
    """z[0] = start, z[i+1] = z[i] * prod_j (v_j[i] + beta id_j[i] + gamma) / prod_j (v_j[i] + beta sigma_j[i] + gamma),
    total = z[n]; d_work holds 2n elements"""
    a = api(is_pallas(ctx))
    assert len(idx_v) == len(idx_id) == len(idx_sigma)
    a.check(a.poly_perm_product_dev(ctx._h, _addr(d_polys), n, n_polys, _idx(idx_v), _idx(idx_id), _idx(idx_sigma), len(idx_v),
                                    _fe(beta), _fe(gamma), _addr(d_start), _addr(d_work), _addr(d_z), _addr(d_total)))
