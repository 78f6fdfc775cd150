"""Many scalar vectors against one resident IPA key (include/snarkv_ipa_batch.h): batched
`IpaProvingKey::commit` and the window table of a key, over a BN254 `Context` + `IpaDecidingKey` or a
pallas `PallasContext` + `PallasIpaDecidingKey`.  The methods `Context.ipa_commit_batch`,
`IpaDecidingKey.prepare` / `.table_bytes` and their pallas twins call into this module.

This ctypes table is this module's own, as `ipa_prover`'s is: one table per header.
"""
import ctypes

from ._bind import bind, is_pallas, signatures
from ._lib import SnarkvError, _as_bytes

_vp, _cp, _sz, _u32, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_dk_prepare": (_int, [_vp, _vp]),
    "ipa_dk_table_bytes": (_sz, [_vp]),
    "ipa_commit_batch": (_int, [_vp, _vp, _cp, _sz, _sz, _vp]),
    "ipa_commit_batch_dev": (_int, [_vp, _vp, _vp, _sz, _sz, _u32, _vp]),
}
# the forms on a library's default context
_CONTEXT_FREE = {
    "bn254_ipa_commit_batch": (_int, [_vp, _cp, _sz, _sz, _vp]),
    "pallas_ipa_commit_batch": (_int, [_vp, _cp, _sz, _sz, _vp]),
}
# every function include/snarkv_ipa_batch.h declares
SIGNATURES = signatures(_SHAPES)
SIGNATURES.update(_CONTEXT_FREE)

SHARED_WINDOWS = 32  # rows of the window table per base: table_bytes = SHARED_WINDOWS * 2^k * 64

def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, {"commit_batch_default": _CONTEXT_FREE}, pallas)


def commit_batch(ctx, dk, polys, n):
    """m commitments in one call: `polys` = m x n canonical scalars (32 bytes LE each, vector after vector),
    1 <= n <= 2^k (the first n bases) -> m points, 64 bytes each, concatenated."""
    a = api(is_pallas(ctx))
    p = _as_bytes(polys)
    if n and len(p) % (32 * n):
        raise SnarkvError(-2, "polys is not a whole number of %d-scalar vectors" % n)
    m = len(p) // (32 * n) if n else 0
    out = ctypes.create_string_buffer(64 * max(m, 1))
    a.check(a.ipa_commit_batch(ctx._h, dk._h, p if p else b"\x00", n, m, out))
    return out.raw[:64 * m]


def commit_batch_dev(ctx, dk, d_polys, n, m, d_out, slices=0):
    """the same from and to device memory, enqueued; `slices` = workgroups per vector (0 = auto)"""
    a = api(is_pallas(ctx))
    a.check(a.ipa_commit_batch_dev(ctx._h, dk._h, _vp(int(d_polys)), n, m, slices, _vp(int(d_out))))


def commit_batch_default(dk, polys, n, pallas):
    """`bn254_ipa_commit_batch` / `pallas_ipa_commit_batch`: on the library's default context"""
    a = api(pallas)
    p = _as_bytes(polys)
    m = len(p) // (32 * n) if n else 0
    out = ctypes.create_string_buffer(64 * max(m, 1))
    a.check(a.commit_batch_default(dk._h, p if p else b"\x00", n, m, out))
    return out.raw[:64 * m]


def dk_prepare(ctx, dk):
    a = api(is_pallas(ctx))
    a.check(a.ipa_dk_prepare(ctx._h, dk._h))


def dk_table_bytes(dk, pallas):
    return int(api(pallas).ipa_dk_table_bytes(dk._h))
