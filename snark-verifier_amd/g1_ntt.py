"""The transform over group elements in device memory (include/snarkv_g1_ntt.h), over a BN254 `Context` or a pallas
`PallasContext`: 2^k points to their combinations with the powers of the domain generator (`ntt_dev`) and back (`intt_dev`),
and the Lagrange basis of a resident IPA key (`dk_lagrange_dev`): the points that commit a column held as evaluations, halo2's
`g_lagrange`.  Every call enqueues on the context's stream and returns; the caller synchronises before it reads a result.

The data are device addresses (ints, or anything with `data_ptr()`): 2^k points of 64 bytes, x || y, the identity all zero.
`d_out` may be `d_in` or disjoint from it.  For every scalar vector v, <v, intt(g)> = <ntt.intt_dev(v), g>.

This ctypes table is this module's own, as `ntt`'s is: one table per header.
"""
import ctypes

from ._bind import addr as _addr, bind, is_pallas, signatures
from .ntt import FORWARD, INVERSE  # noqa: F401  (SNARKV_NTT_FORWARD, SNARKV_NTT_INVERSE)

_vp, _int, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "g1_ntt_dev": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "ipa_dk_lagrange_dev": (_int, [_vp, _vp, _vp]),
    "g1_ntt_max_k": (_u32, []),
}
# every function include/snarkv_g1_ntt.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def _transform(ctx, d_in, d_out, k, direction):
    a = api(is_pallas(ctx))
    a.check(a.g1_ntt_dev(ctx._h, _addr(d_in), _addr(d_out), k, direction))


def ntt_dev(ctx, d_in, d_out, k):
    """out[i] = sum_j w^(i j) in[j]"""
    _transform(ctx, d_in, d_out, k, FORWARD)


def intt_dev(ctx, d_in, d_out, k):
    """out[i] = n^-1 sum_j w^(-i j) in[j]: a key's points to its Lagrange basis"""
    _transform(ctx, d_in, d_out, k, INVERSE)


def dk_lagrange_dev(ctx, dk, d_out):
    """the Lagrange basis of a whole resident key (`IpaDecidingKey`, `ipa_dk_create`): 2^k points to `d_out`"""
    a = api(is_pallas(ctx))
    a.check(a.ipa_dk_lagrange_dev(ctx._h, dk._h, _addr(d_out)))


def max_k(ctx):
    """the largest k of the context's library"""
    return int(api(is_pallas(ctx)).g1_ntt_max_k())
