"""The IPA prover on the device (include/snarkv_ipa_prover.h): `Ipa::create_proof` and
`IpaAs::create_proof` (reference snark-verifier/src/pcs/ipa.rs:39-124,
pcs/ipa/accumulation.rs:148-226) over a BN254 `Context` + `IpaDecidingKey` or a pallas
`PallasContext` + `PallasIpaDecidingKey`.

The device runs the rounds (inner products, MSMs, the folds) and the h-combination of `IpaAs`; this
module drives the transcript, as a Rust `TranscriptWrite` would.  Scalars are ints, points (x, y)
int pairs with None for the identity.  A transcript is any object with `write_ec_point`,
`write_scalar`, `common_ec_point`, `common_scalar` and `squeeze_challenge`.  `rng()` returns a fresh
scalar (plays `C::Scalar::random`); it is called in the reference's order.

This ctypes table is this module's own: the header is not snarkv_amd.h, whose table is `_lib._SIGNATURES`.
"""
import ctypes

from ._bind import bind, fe as _fe, is_pallas, signatures
from ._lib import _as_bytes

_vp, _cp, _sz, _u32, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "ipa_commit": (_int, [_vp, _vp, _cp, _sz, _cp, _cp, _vp]),
    "ipa_prover_begin": (_int, [_vp, _vp, _cp, _sz, _cp, _cp, _cp, ctypes.POINTER(_vp)]),
    "ipa_prover_begin_dev": (_int, [_vp, _vp, _vp, _sz, _cp, _cp, _cp, ctypes.POINTER(_vp)]),
    "ipa_prover_round": (_int, [_vp, _vp, _vp]),
    "ipa_prover_fold": (_int, [_vp, _cp]),
    "ipa_prover_finish": (_int, [_vp, _vp, _vp]),
    "ipa_prover_destroy": (None, [_vp]),
    "ipa_as_combine_dev": (_int, [_vp, _cp, _sz, _u32, _cp, _cp, _vp]),
}
# every function include/snarkv_ipa_prover.h declares, for both libraries
SIGNATURES = signatures(_SHAPES)

# scalar field orders: BN254 r and pallas q (include/snarkv_pallas.h)
R_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
R_PALLAS = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001

def _api(ctx):
    """the prover functions of the context's library, with its modulus as `.r`"""
    pallas = is_pallas(ctx)
    a = bind(_SHAPES, None, pallas)
    a.r = R_PALLAS if pallas else R_BN254
    return a


def _pt(p):
    return b"\x00" * 64 if p is None else _fe(p[0]) + _fe(p[1])


def _from_pt(b):
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")
    return None if x == 0 and y == 0 else (x, y)


def commit(ctx, dk, poly, omega=None, s=None):
    """`IpaProvingKey::commit` (ipa.rs:221-229) with the resident key: sum poly[j] G[j] (+ omega s); `poly` may be
    shorter than the key (the first len(poly) bases).  Returns the point."""
    api = _api(ctx)
    pb = b"".join(_fe(c % api.r) for c in poly)
    out = ctypes.create_string_buffer(64)
    om = None if omega is None else _fe(omega % api.r)
    sb = None if omega is None else _pt(s)
    api.check(api.ipa_commit(ctx._h, dk._h, pb, len(poly), om, sb, out))
    return _from_pt(out.raw)


def as_combine_dev(ctx, xis, alpha, ab, d_h):
    """h = sum_i alpha^i h_coeffs(xi_i) (+ alpha^m (b, a, 0, ...) when `ab` = (a, b)) into device memory `d_h`
    (2^k x 32 bytes): `snarkv_ipa_as_combine_dev`."""
    api = _api(ctx)
    k = len(xis[0])
    assert all(len(x) == k for x in xis)
    xb = b"".join(_fe(x) for xi in xis for x in xi)
    abb = None if ab is None else _fe(ab[0]) + _fe(ab[1])
    api.check(api.ipa_as_combine_dev(ctx._h, xb, len(xis), k, _fe(alpha), abb, ctypes.c_void_p(int(d_h))))


class IpaProver:
    """One `snarkv_ipa_prover` session: `round()` then `fold(xi)`, k times each, then `finish()`.

    `coeffs`: the 2^k coefficients of p' as bytes (32 each), or a device pointer (int) with `n`."""

    def __init__(self, ctx, dk, coeffs, z, h, xi0, n=None):
        self._api = _api(ctx)
        self._h = _vp()
        self.k = dk.k
        zb, hb, xb = _fe(z), _pt(h), _fe(xi0)
        if isinstance(coeffs, int):
            assert n is not None
            rc = self._api.ipa_prover_begin_dev(ctx._h, dk._h, _vp(coeffs), n, zb, hb, xb, ctypes.byref(self._h))
        else:
            cb = _as_bytes(coeffs)
            rc = self._api.ipa_prover_begin(ctx._h, dk._h, cb if cb else b"\x00", len(cb) // 32, zb, hb, xb,
                                            ctypes.byref(self._h))
        self._api.check(rc)

    def round(self):
        """(L_i, R_i) as 64-byte points"""
        l, r = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        self._api.check(self._api.ipa_prover_round(self._h, l, r))
        return l.raw, r.raw

    def fold(self, xi):
        self._api.check(self._api.ipa_prover_fold(self._h, xi if isinstance(xi, bytes) else _fe(xi)))

    def finish(self):
        """(U, c): the last base (64 bytes) and the last coefficient (32 bytes)"""
        u, c = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        self._api.check(self._api.ipa_prover_finish(self._h, u, c))
        return u.raw, c.raw

    def close(self):
        if self._h:
            self._api.ipa_prover_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _poly_eval(coeffs, z, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % r
    return acc


def _device_bytes(ctx, nbytes):
    import torch

    return torch.empty(nbytes, dtype=torch.uint8, device="cuda:%d" % getattr(ctx, "device", 0))


def _prove(ctx, dk, h, s, p, d_p, z, omega, transcript, rng):
    """ipa.rs:39-124 with p' either on the host (`p`, ints) or on the device (`d_p`, a uint8 tensor)."""
    api = _api(ctx)
    r = api.r
    n = 1 << dk.k
    if s is not None:
        if p is None:  # p' = p + alpha p_bar is a host loop, as in the reference: bring p back
            raw = bytes(d_p.cpu().numpy().tobytes())
            p = [int.from_bytes(raw[32 * j:32 * j + 32], "little") for j in range(n)]
        p_bar = [rng() for _ in range(n)]
        p_bar[0] = (p_bar[0] - _poly_eval(p_bar, z, r)) % r
        omega_bar = rng()
        transcript.write_ec_point(commit(ctx, dk, p_bar, omega_bar, s))
        alpha = transcript.squeeze_challenge()
        transcript.write_scalar((omega + alpha * omega_bar) % r)
        p = [(a + alpha * b) % r for a, b in zip(p, p_bar)]
    xi_0 = transcript.squeeze_challenge()
    if p is not None:
        assert len(p) == n
        src = b"".join(_fe(c % r) for c in p)
        prover = IpaProver(ctx, dk, src, z, h, xi_0)
    else:
        prover = IpaProver(ctx, dk, d_p.data_ptr(), z, h, xi_0, n=n)
    xi = []
    with prover:
        for _ in range(dk.k):
            l_i, r_i = prover.round()
            transcript.write_ec_point(_from_pt(l_i))
            transcript.write_ec_point(_from_pt(r_i))
            x = transcript.squeeze_challenge()
            prover.fold(x)
            xi.append(x)
        u, c = prover.finish()
    u = _from_pt(u)
    transcript.write_ec_point(u)
    transcript.write_scalar(int.from_bytes(c, "little"))
    return xi, u


def create_proof(ctx, dk, h, s, p, z, omega, transcript, rng):
    """`Ipa::create_proof` (ipa.rs:39-124) for the key (dk, h, s): `s` None is the non-zk key (then `omega` is None).
    Returns the accumulator (xi, U)."""
    return _prove(ctx, dk, h, s, list(p), None, z, omega, transcript, rng)


def as_create_proof(ctx, dk, h, s, accumulators, transcript, rng):
    """`IpaAs::create_proof` (accumulation.rs:148-226) over `accumulators` = [(xi, U), ...] (at least two).
    Returns the new accumulator (xi, U)."""
    assert len(accumulators) > 1
    api = _api(ctx)
    ab = omega = None
    if s is not None:
        a, b = rng(), rng()
        u = commit(ctx, dk, [b, a])  # g[1] a + g[0] b
        transcript.write_scalar(a)
        transcript.write_scalar(b)
        transcript.write_ec_point(u)
        ab = (a, b)
        omega = rng()
        transcript.write_scalar(omega)
    for xi, u in accumulators:
        for x in xi:
            transcript.common_scalar(x)
        transcript.common_ec_point(u)
    alpha = transcript.squeeze_challenge()
    z = transcript.squeeze_challenge()
    d_h = _device_bytes(ctx, 32 << dk.k)
    as_combine_dev(ctx, [xi for xi, _ in accumulators], alpha % api.r, ab, d_h.data_ptr())
    return _prove(ctx, dk, h, s, None, d_h, z, omega, transcript, rng)
