"""A PLONK prover on pallas through the product API of the host mirror (include/snarkv_host_pallas_plonk_prove.h,
libsnarkv_host_pallas_plonk_prove.so): a `host_api_pallas.Protocol`, a resident IPA key of a `PallasContext` and the witness
polynomials in device memory in, proof bytes and the opening's accumulator out -- halo2's IPA backend: blinded commitments, the
Bgh19 multi-open, the Blake2b transcript.

    with PlonkProver(protocol, ctx, dk, h, s, d_preprocessed, pre_blinds, instances) as p:
        challenges = p.phase(d_advice, advice_blinds)              # one call per entry of the protocol's num_witness
        challenges += p.phase(None)                                # a phase without witnesses
        challenges += p.phase(d_z, z_blinds, form=FORM_VALUES)     # made from the challenges so far
        proof, acc = p.finish(chunk_blinds, f_blind, d_pbar, omega_bar)   # (None, None): the witness does not satisfy

Blinds are ints or 32-byte scalars, one per polynomial; every bit of randomness is the caller's, so a proof is a function of
the arguments.  `plan(protocol)` needs no device: what the protocol compiles to, or the refusal as a `HostError`.
`flags=QUOTIENT_COSETS` as in `host_plonk_prove`.

The ctypes table is this module's own: one table per header."""
import ctypes
import os

from . import host_api_pallas as H
from ._bind import Api, addr as _addr, fe as _fe, scalars as _scalars

_vp, _cp, _sz, _int, _u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
_szp = ctypes.POINTER(_sz)

FORM_COEFFS, FORM_VALUES = 0, 1
UNSATISFIED = "the witness does not satisfy the protocol's constraints"
QUOTIENT_COSETS = 1  # SNARKV_HOST_PALLAS_PLONK_QUOTIENT_COSETS

LIB_NAME = "libsnarkv_host_pallas_plonk_prove.so"
PREFIX = "snarkv_host_pallas_plonk_prover_"
# every function include/snarkv_host_pallas_plonk_prove.h declares, without the prefix
SHAPES = {
    "last_error": (_cp, []),
    "plan": (_int, [_vp, _u32, ctypes.POINTER(_u32), _szp, _szp, _szp, _szp]),
    "begin": (_int, [_vp, _u32, _vp, _vp, _cp, _cp, _vp, _cp, _cp, _sz, ctypes.POINTER(_vp)]),
    "phase": (_int, [_vp, _vp, _int, _cp, _vp, _sz, _szp]),
    "finish": (_int, [_vp, _cp, _cp, _vp, _cp, _vp, _sz, _szp, _vp]),
    "destroy": (None, [_vp]),
}
SIGNATURES = {PREFIX + n: s for n, s in SHAPES.items()}
_bound = None


def lib_path():
    return os.environ.get("SNARKV_HOST_PALLAS_PLONK_PROVE_LIB") or os.path.join(H.HERE, LIB_NAME)


def api():
    """the functions of the header, bound once: `api().begin` is snarkv_host_pallas_plonk_prover_begin.  No fallback: a
    missing library raises."""
    global _bound
    if _bound is None:
        path = lib_path()
        if not os.path.exists(path):
            raise H.HostError(H.ERR_DEVICE, "%s not built (run `python __graft_entry__.py`)" % path)
        H.load_library()  # libsnarkv_pallas.so and libsnarkv_host_pallas.so first, through their own loaders
        _bound = Api(ctypes.CDLL(path), PREFIX, SHAPES)  # AttributeError if the header and the library drift
    return _bound


def last_error():
    return api().last_error()


def _check(rc):
    if rc < 0:
        raise H.HostError(rc, last_error())
    return rc


def pack_instances(instances):
    """[[int]] -> one packed instance block"""
    out = len(instances).to_bytes(4, "little")
    for column in instances:
        out += len(column).to_bytes(4, "little") + b"".join(int(v).to_bytes(32, "little") for v in column)
    return out


def _blinds(blinds):
    """one scalar per polynomial, ints or 32 bytes each; None (no polynomial) stays None"""
    return None if blinds is None else _scalars(list(blinds))


def plan(protocol, flags=0):
    """-> {"e", "n_cols", "n_instr", "n_consts", "bytes"}; a protocol the prover refuses raises HostError naming the cause.
    `bytes` is what a session begun with the same `flags` allocates."""
    e, cols, instr, consts, nbytes = _u32(0), _sz(0), _sz(0), _sz(0), _sz(0)
    _check(api().plan(protocol._h, flags, ctypes.byref(e), ctypes.byref(cols), ctypes.byref(instr), ctypes.byref(consts),
                      ctypes.byref(nbytes)))
    return {"e": e.value, "n_cols": cols.value, "n_instr": instr.value, "n_consts": consts.value, "bytes": nbytes.value}


class PlonkProver:
    """A prover session.  `ctx`: a `PallasContext`; `dk`: its resident key of 2^k points (`ctx.ipa_dk_create`); `h`, `s`: the
    key's two other points, 64 bytes each.  `instances`: [[int]] or a packed block.  The key and whatever a phase is given stay
    the caller's; the session keeps its own copy of every polynomial."""

    _api = staticmethod(api)  # the library of the session's six calls (host_plonk_prove_pallas_ci binds another)

    def _check(self, rc):
        if rc < 0:
            raise H.HostError(rc, self._a.last_error())
        return rc

    def __init__(self, protocol, ctx, dk, h, s, d_preprocessed, pre_blinds, instances, flags=0):
        self._a, self._h = self._api(), None
        inst = bytes(instances) if isinstance(instances, (bytes, bytearray)) else pack_instances(instances)
        hd = _vp()
        self._check(self._a.begin(protocol._h, flags, ctx._h, dk._h, None if h is None else bytes(h), None if s is None else bytes(s),
                             _addr(d_preprocessed), _blinds(pre_blinds), inst, len(inst), ctypes.byref(hd)))
        self._h, self._keep, self.k = hd, (protocol, ctx, dk), dk.k

    def phase(self, d_witness, blinds=None, form=FORM_COEFFS):
        """the next phase's polynomials and their blinds (None for a phase without any) -> the challenges squeezed after
        them, as ints"""
        n = _sz(0)
        out = ctypes.create_string_buffer(32 * 64)
        self._check(self._a.phase(self._h, _addr(d_witness), form, _blinds(blinds), out, 64, ctypes.byref(n)))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n.value)]

    def finish(self, chunk_blinds, f_blind, d_pbar, omega_bar):
        """-> (proof bytes, accumulator bytes: k x xi | u), or (None, None) when the witness does not satisfy the protocol's
        constraints"""
        n = _sz(0)
        rc = self._a.finish(self._h, None, None, None, None, None, 0, ctypes.byref(n), None)
        if rc != H.ERR_CAPACITY:
            self._check(rc)
            raise H.HostError(H.ERR_OTHER, "finish: a proof of no bytes")
        out, acc = ctypes.create_string_buffer(n.value), ctypes.create_string_buffer(32 * self.k + 64)
        rc = self._check(self._a.finish(self._h, _blinds(chunk_blinds), _fe(f_blind), _addr(d_pbar), _fe(omega_bar), out, len(out),
                                   ctypes.byref(n), acc))
        return (out.raw[:n.value], acc.raw) if rc == 1 else (None, None)

    def close(self):
        if self._h:
            self._a.destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
