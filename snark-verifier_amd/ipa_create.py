"""`Ipa::create_proof` in one call with halo2's Blake2b transcript on the device (include/snarkv_ipa_create.h), over a
BN254 `Context` + `IpaDecidingKey` or a pallas `PallasContext` + `PallasIpaDecidingKey`: the proof bytes a `Blake2bRead`
reads and the accumulator (xi, U).  `ipa_prover.create_proof` drives the same rounds through the session with a host
transcript of any kind; this call keeps the transcript on the device and synchronises once.

Scalars are ints or 32-byte strings, vectors lists of ints or packed bytes, points (x, y) int pairs or 64-byte strings.
The zero-knowledge branch is taken when `s`, `omega`, `p_bar` and `omega_bar` are all given: `p_bar` and `omega_bar` are
what the reference draws from its rng (n scalars, then one), in that order.

This ctypes table is this module's own, as `ipa_fold`'s is: one table per header.
"""
import ctypes

from ._bind import bind, fe as _fe, is_pallas, prove, pt as _pt, signatures, vec as _vec

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_szp = ctypes.POINTER(ctypes.c_size_t)

_TAIL = [_cp, _sz, _vp, _sz, _szp, _vp, _vp]  # absorbed, its length, proof_out, proof_cap, proof_len, xi_out, u_out
# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_create_proof": (_int, [_vp, _vp, _cp, _cp, _cp, _sz, _cp, _cp, _cp, _cp] + _TAIL),
    "ipa_create_proof_dev": (_int, [_vp, _vp, _cp, _cp, _vp, _sz, _cp, _cp, _vp, _cp] + _TAIL),
}
# the forms on a library's default context
_CONTEXT_FREE = {
    "bn254_ipa_create_proof": (_int, [_vp, _cp, _cp, _cp, _sz, _cp, _cp, _cp, _cp] + _TAIL),
    "pallas_ipa_create_proof": (_int, [_vp, _cp, _cp, _cp, _sz, _cp, _cp, _cp, _cp] + _TAIL),
}
# every function include/snarkv_ipa_create.h declares
SIGNATURES = signatures(_SHAPES)
SIGNATURES.update(_CONTEXT_FREE)

def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, {"create_proof_default": _CONTEXT_FREE}, pallas)


def proof_bytes(k, zk):
    """the length of a proof: 64 k + 64, + 64 with the zero-knowledge branch"""
    return 64 * k + 64 + (64 if zk else 0)


def _prove(a, fn, handles, dk, h, s, p, n, z, omega, p_bar, omega_bar, absorbed):
    """`p` and `p_bar` as the call takes them: packed bytes or device addresses"""
    return prove(a, fn, dk.k, proof_bytes(dk.k, True), *handles, _pt(h), _pt(s), p, n, _fe(z), _fe(omega), p_bar,
                 _fe(omega_bar), bytes(absorbed) or None, len(absorbed))


def create_proof(ctx, dk, h, s, p, z, omega=None, p_bar=None, omega_bar=None, absorbed=b""):
    """-> (proof bytes, (xi, U)).  `absorbed`: the raw bytes the transcript's hasher has taken before the proof."""
    a, pb = api(is_pallas(ctx)), _vec(p)
    return _prove(a, a.ipa_create_proof, (ctx._h, dk._h), dk, h, s, pb if pb else b"\x00", len(pb) // 32, z, omega, _vec(p_bar),
                  omega_bar, absorbed)


def create_proof_dev(ctx, dk, h, s, d_p, n, z, omega=None, d_p_bar=None, omega_bar=None, absorbed=b""):
    """the same with the coefficients (and p_bar) at device addresses: n x 32 bytes each"""
    a = api(is_pallas(ctx))
    return _prove(a, a.ipa_create_proof_dev, (ctx._h, dk._h), dk, h, s, _vp(int(d_p)), n, z, omega,
                  None if d_p_bar is None else _vp(int(d_p_bar)), omega_bar, absorbed)


def create_proof_default(dk, h, s, p, z, omega=None, p_bar=None, omega_bar=None, absorbed=b"", pallas=False):
    """`bn254_ipa_create_proof` / `pallas_ipa_create_proof`: on the library's default context"""
    a, pb = api(pallas), _vec(p)
    return _prove(a, a.create_proof_default, (dk._h,), dk, h, s, pb if pb else b"\x00", len(pb) // 32, z, omega, _vec(p_bar),
                  omega_bar, absorbed)
