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

from ._lib import SnarkvError, _as_bytes

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
SIGNATURES = {p + n: s for p in ("snarkv_", "snarkv_pallas_") for n, s in _SHAPES.items()}
SIGNATURES.update(_CONTEXT_FREE)

_BOUND = {}


class _Api:
    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        free = ("pallas" if prefix == "snarkv_pallas_" else "bn254") + "_ipa_create_proof"
        for name, (res, args) in [(prefix + n, s) for n, s in _SHAPES.items()] + [(free, _CONTEXT_FREE[free])]:
            fn = getattr(lib, name)  # AttributeError if the header and the library drift
            fn.restype, fn.argtypes = res, args
        self.create_proof_default = getattr(lib, free)

    def __getattr__(self, name):
        return getattr(self.lib, self.prefix + name)

    def check(self, rc):
        if rc < 0:
            err = self.lib.snarkv_pallas_last_error if self.prefix == "snarkv_pallas_" else self.lib.snarkv_last_error
            raise SnarkvError(rc, (err() or b"").decode(errors="replace"))
        return rc


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    if pallas not in _BOUND:
        if pallas:
            from .pallas import load_library

            _BOUND[pallas] = _Api(load_library(), "snarkv_pallas_")
        else:
            from ._lib import load_library

            _BOUND[pallas] = _Api(load_library(), "snarkv_")
    return _BOUND[pallas]


def _is_pallas(ctx):
    from .pallas import PallasContext

    return isinstance(ctx, PallasContext)


def _fe(v):
    return None if v is None else (int(v).to_bytes(32, "little") if isinstance(v, int) else _as_bytes(v))


def _pt(p):
    if p is None or isinstance(p, (bytes, bytearray)):
        return p
    return int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little")


def _vec(v):
    if v is None or isinstance(v, (bytes, bytearray)):
        return v
    return b"".join(int(c).to_bytes(32, "little") for c in v)


def proof_bytes(k, zk):
    """the length of a proof: 64 k + 64, + 64 with the zero-knowledge branch"""
    return 64 * k + 64 + (64 if zk else 0)


def _finish(a, k, rc, proof, plen, xi, u):
    a.check(rc)
    xis = [int.from_bytes(xi.raw[32 * i:32 * i + 32], "little") for i in range(k)]
    x, y = int.from_bytes(u.raw[:32], "little"), int.from_bytes(u.raw[32:], "little")
    return proof.raw[:plen.value], (xis, (x, y))


def _outs(k):
    cap = proof_bytes(k, True)
    return ctypes.create_string_buffer(cap), cap, ctypes.c_size_t(0), ctypes.create_string_buffer(32 * max(k, 1)), \
        ctypes.create_string_buffer(64)


def create_proof(ctx, dk, h, s, p, z, omega=None, p_bar=None, omega_bar=None, absorbed=b""):
    """-> (proof bytes, (xi, U)).  `absorbed`: the raw bytes the transcript's hasher has taken before the proof."""
    a = api(_is_pallas(ctx))
    pb = _vec(p)
    proof, cap, plen, xi, u = _outs(dk.k)
    rc = a.ipa_create_proof(ctx._h, dk._h, _pt(h), _pt(s), pb if pb else b"\x00", len(pb) // 32, _fe(z), _fe(omega),
                            _vec(p_bar), _fe(omega_bar), bytes(absorbed) or None, len(absorbed), proof, cap,
                            ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)


def create_proof_dev(ctx, dk, h, s, d_p, n, z, omega=None, d_p_bar=None, omega_bar=None, absorbed=b""):
    """the same with the coefficients (and p_bar) at device addresses: n x 32 bytes each"""
    a = api(_is_pallas(ctx))
    proof, cap, plen, xi, u = _outs(dk.k)
    rc = a.ipa_create_proof_dev(ctx._h, dk._h, _pt(h), _pt(s), _vp(int(d_p)), n, _fe(z), _fe(omega),
                                None if d_p_bar is None else _vp(int(d_p_bar)), _fe(omega_bar), bytes(absorbed) or None,
                                len(absorbed), proof, cap, ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)


def create_proof_default(dk, h, s, p, z, omega=None, p_bar=None, omega_bar=None, absorbed=b"", pallas=False):
    """`bn254_ipa_create_proof` / `pallas_ipa_create_proof`: on the library's default context"""
    a = api(pallas)
    pb = _vec(p)
    proof, cap, plen, xi, u = _outs(dk.k)
    rc = a.create_proof_default(dk._h, _pt(h), _pt(s), pb if pb else b"\x00", len(pb) // 32, _fe(z), _fe(omega), _vec(p_bar),
                                _fe(omega_bar), bytes(absorbed) or None, len(absorbed), proof, cap, ctypes.byref(plen), xi, u)
    return _finish(a, dk.k, rc, proof, plen, xi, u)
