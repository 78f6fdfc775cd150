"""`IpaAs::decide_all` as one folded check over a random linear combination (include/snarkv_ipa_fold.h):
`sum rho^i U_i == <sum rho^i h_coeffs(xi_i), G>`, over a BN254 `Context` + `IpaDecidingKey` or a pallas
`PallasContext` + `PallasIpaDecidingKey`.  The methods `Context.ipa_decide_folded`,
`Context.ipa_fold_coeffs_dev` and their pallas twins call into this module.

These calls take rho from the caller, who owns its soundness: it must be unpredictable to whoever chose the
accumulators (`fold_challenge` below derives one from the accumulators themselves).

This ctypes table is this module's own, as `ipa_batch`'s is: one table per header.
"""
import ctypes
import hashlib

from ._bind import bind, is_pallas, signatures
from ._lib import SnarkvError, _as_bytes

_vp, _cp, _sz, _u32, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
_ip = ctypes.POINTER(ctypes.c_int)

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_fold_coeffs_dev": (_int, [_vp, _u32, _cp, _sz, _cp, _u32, _vp]),
    "ipa_decide_folded": (_int, [_vp, _vp, _cp, _cp, _sz, _cp, _ip]),
}
# the forms on a library's default context
_CONTEXT_FREE = {
    "bn254_ipa_decide_folded": (_int, [_vp, _cp, _cp, _sz, _cp, _ip]),
    "pallas_ipa_decide_folded": (_int, [_vp, _cp, _cp, _sz, _cp, _ip]),
}
# every function include/snarkv_ipa_fold.h declares
SIGNATURES = signatures(_SHAPES)
SIGNATURES.update(_CONTEXT_FREE)

FOLD_BLOCK_BITS = 3  # a lane of the fold kernel owns 2^3 consecutive coefficients (csrc/ipa_fold.h kFoldT)

R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
R_PALLAS = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001

def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, {"decide_folded_default": _CONTEXT_FREE}, pallas)


def _split(k, xi, u):
    xi, u = _as_bytes(xi), _as_bytes(u)
    m = len(u) // 64
    if len(u) != 64 * m or len(xi) != 32 * k * m:
        raise SnarkvError(-2, "xi / u are not m x k scalars and m points")
    return xi, u, m


def _rho(rho):
    rho = _as_bytes(rho) if not isinstance(rho, int) else rho.to_bytes(32, "little")
    if len(rho) != 32:
        raise SnarkvError(-2, "rho is one 32-byte scalar")
    return rho


def decide_folded(ctx, dk, xi, u, rho):
    """True iff `sum rho^i U_i == <sum rho^i h_coeffs(xi_i), G>`: `xi` = m x k scalars (32 bytes LE each), `u` = m points
    (64 bytes each), `rho` = 32 bytes LE or an int.  An off-curve or non-canonical U is False, not an exception."""
    a = api(is_pallas(ctx))
    xi, u, m = _split(dk.k, xi, u)
    ok = ctypes.c_int(0)
    a.check(a.ipa_decide_folded(ctx._h, dk._h, xi if xi else b"\x00", u if u else b"\x00", m, _rho(rho), ctypes.byref(ok)))
    return ok.value != 0


def decide_folded_default(dk, xi, u, rho, pallas):
    """`bn254_ipa_decide_folded` / `pallas_ipa_decide_folded`: on the library's default context"""
    a = api(pallas)
    xi, u, m = _split(dk.k, xi, u)
    ok = ctypes.c_int(0)
    a.check(a.decide_folded_default(dk._h, xi if xi else b"\x00", u if u else b"\x00", m, _rho(rho), ctypes.byref(ok)))
    return ok.value != 0


def fold_coeffs_dev(ctx, k, xi, rho, d_h, slices=0):
    """`sum rho^i h_coeffs(xi_i)` as 2^k canonical scalars at device address `d_h` (16-byte aligned), enqueued;
    `slices` = accumulator slices per coefficient block (0 = auto)"""
    a = api(is_pallas(ctx))
    xi = _as_bytes(xi)
    if k < 1 or len(xi) % (32 * k):
        raise SnarkvError(-2, "xi is not a whole number of %d-scalar challenge vectors" % k)
    m = len(xi) // (32 * k)
    a.check(a.ipa_fold_coeffs_dev(ctx._h, k, xi if xi else b"\x00", m, _rho(rho), slices, _vp(int(d_h))))


def fold_challenge(k, xi, u, pallas, seed=None):
    """A rho for `decide_folded`, derived on the host from the accumulators it weighs (no device work): BLAKE2b-512 with
    the personalisation `snarkv_ipa_fold1` over `u32le k | u32le m | the m accumulators, k x xi | u each | the 32 seed
    bytes if given`, the digest read little-endian and reduced mod r (as halo2's Blake2b transcript squeezes) -> 32 bytes
    LE.  `seed`: the verifier's own randomness, optional."""
    xi, u, m = _split(k, xi, u)
    if seed is not None and len(seed) != 32:
        raise SnarkvError(-2, "seed is 32 bytes")
    h = hashlib.blake2b(digest_size=64, person=b"snarkv_ipa_fold1")
    h.update(k.to_bytes(4, "little") + m.to_bytes(4, "little"))
    for a in range(m):
        h.update(xi[32 * k * a:32 * k * (a + 1)] + u[64 * a:64 * (a + 1)])
    if seed is not None:
        h.update(bytes(seed))
    return (int.from_bytes(h.digest(), "little") % (R_PALLAS if pallas else R_BN254)).to_bytes(32, "little")
