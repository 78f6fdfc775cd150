"""The number-theoretic transform over the scalar field on polynomials in device memory (include/snarkv_ntt.h), over a BN254
`Context` or a pallas `PallasContext`: coefficients to evaluations over the 2^k domain or a coset of it (`ntt_dev`) and back
(`intt_dev`), natural order on both sides.  Every call enqueues on the context's stream and returns; the caller synchronises
before it reads a result.

The data are device addresses (ints, or anything with `data_ptr()`): `count` polynomials of 2^k elements of 32 bytes each,
poly-major.  `d_out` may be `d_in` or disjoint from it.  `shift` is an int or 32 bytes; `intt_dev` with the shift s^-1 undoes
`ntt_dev` with the shift s.

This ctypes table is this module's own, as `poly`'s is: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, fe as _fe, is_pallas, signatures

_vp, _cp, _sz, _int, _u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32

TILE_BITS = 9  # log2 of the elements of a tile, the levels one pass takes at most (csrc/ntt.hip: kNttTileBits)
COL_BITS = 2  # with several passes a pass takes at most TILE_BITS - COL_BITS levels (kNttColBits)
REDUCE_EVERY = 6  # levels between two reductions of the lazy sums (csrc/ntt_tile.h: kNttReduceEvery)
FORWARD, INVERSE = 0, 1  # SNARKV_NTT_FORWARD, SNARKV_NTT_INVERSE
MAX_COUNT = 65535

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ntt_dev": (_int, [_vp, _vp, _vp, _u32, _sz, _u32, _cp]),
    "ntt_max_k": (_u32, []),
}
# every function include/snarkv_ntt.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def passes(k):
    """how many passes a transform of 2^k takes (csrc/ntt_plan.h)"""
    return 1 if k <= TILE_BITS else -(-k // (TILE_BITS - COL_BITS))


def _transform(ctx, d_in, d_out, k, count, direction, shift):
    a = api(is_pallas(ctx))
    a.check(a.ntt_dev(ctx._h, _addr(d_in), _addr(d_out), k, count, direction, _fe(shift)))


def ntt_dev(ctx, d_in, d_out, k, count=1, shift=None):
    """out[i] = sum_j (shift^j in[j]) w^(i j): the values on the coset shift * H of the 2^k domain"""
    _transform(ctx, d_in, d_out, k, count, FORWARD, shift)


def intt_dev(ctx, d_in, d_out, k, count=1, shift=None):
    """out[j] = shift^j n^-1 sum_i in[i] w^(-i j): the coefficients, 1/n included"""
    _transform(ctx, d_in, d_out, k, count, INVERSE, shift)


def max_k(ctx):
    """the largest k of the context's library: min(two-adicity of the scalar field, 30)"""
    return int(api(is_pallas(ctx)).ntt_max_k())
