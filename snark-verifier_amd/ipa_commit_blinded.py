"""Many blinded commitments against one resident IPA key (include/snarkv_ipa_commit_blinded.h):
`out[a] = <polys[a], G> + blinds[a] * S`, over a BN254 `Context` + `IpaDecidingKey` or a pallas `PallasContext` +
`PallasIpaDecidingKey`.

This ctypes table is this module's own, as `ipa_batch`'s is: one table per header.
"""
import ctypes

from ._bind import addr, bind, is_pallas, pt, signatures, vec

_vp, _cp, _sz, _u32, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_commit_blinded_batch_dev": (_int, [_vp, _vp, _cp, _vp, _sz, _sz, _cp, _u32, _vp]),
}
# every function include/snarkv_ipa_commit_blinded.h declares
SIGNATURES = signatures(_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def commit_blinded_batch_dev(ctx, dk, s, d_polys, n, m, blinds, d_out, slices=0):
    """m blinded commitments from and to device memory, enqueued on the context's stream: `s` = the point S (an (x, y)
    pair or 64 bytes), `blinds` = m scalars (ints or packed bytes) on the host, `slices` = workgroups per vector (0 = auto)"""
    a = api(is_pallas(ctx))
    a.check(a.ipa_commit_blinded_batch_dev(ctx._h, dk._h, pt(s), addr(d_polys), n, m, vec(blinds), slices, addr(d_out)))
