"""The lookup argument on resident columns (include/snarkv_lookup.h), over a BN254 `Context` or a pallas `PallasContext`:
the sort of a column of scalars (`sort_dev`), halo2's permute_expression_pair (`permute_dev`: the permuted input and table
columns and a status) and the lookup product Z (`product_dev`).  Every call enqueues on the context's stream and returns; the
caller synchronises before it reads a result, the status included.

Columns, work buffers, start values, totals and the status are device addresses (ints, or anything with `data_ptr()`);
column indices are ints and the challenges ints or 32-byte strings.

This ctypes table is this module's own, as `poly_prod`'s and `quotient`'s are: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, fe as _fe, is_pallas, signatures

_vp, _cp, _sz, _int, _u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32

TILE = 1024  # SNARKV_LOOKUP_TILE: elements per sort tile and per merge chunk (csrc/lookup.hip: kLkTile)
SCAN_BLOCK = 1024  # SNARKV_LOOKUP_SCAN_BLOCK: rows per block of the count scans at level 0 (kLkScanBlock)
SCAN_LEVEL_BLOCK = 1024  # ... and at the levels above: the same
STATUS_BYTES = 16  # four uint32: missing distinct input values, distinct input values, 0, 0

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "poly_sort_dev": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "lookup_permute_dev": (_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "lookup_product_dev": (_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _cp, _cp, _vp, _vp, _vp, _vp]),
}
# every function include/snarkv_lookup.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def sort_dev(ctx, d_in, n, d_work, d_out):
    """out = in sorted ascending by the canonical value; d_work holds n elements; out may be in"""
    a = api(is_pallas(ctx))
    a.check(a.poly_sort_dev(ctx._h, _addr(d_in), n, _addr(d_work), _addr(d_out)))


def permute_dev(ctx, d_input, d_table, u, d_work, d_perm_input, d_perm_table, d_status):
    """halo2's permute_expression_pair over the first u rows: perm_input = the sorted input, perm_table = the table arranged
    against it; d_work holds 2u elements, d_status 16 bytes (status[0] = distinct input values the table lacks)"""
    a = api(is_pallas(ctx))
    a.check(a.lookup_permute_dev(ctx._h, _addr(d_input), _addr(d_table), u, _addr(d_work), _addr(d_perm_input),
                                 _addr(d_perm_table), _addr(d_status)))


def product_dev(ctx, d_polys, n, n_polys, idx_input, idx_table, idx_perm_input, idx_perm_table, beta, gamma, d_work, d_z,
                d_start=None, d_total=None):
    """z[0] = start, z[i+1] = z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)), total = z[n]; d_work holds
    2n elements"""
    a = api(is_pallas(ctx))
    a.check(a.lookup_product_dev(ctx._h, _addr(d_polys), n, n_polys, idx_input, idx_table, idx_perm_input, idx_perm_table,
                                 _fe(beta), _fe(gamma), _addr(d_start), _addr(d_work), _addr(d_z), _addr(d_total)))
