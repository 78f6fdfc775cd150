"""A PLONK prover through the product API of the host mirror (include/snarkv_host_plonk_prove.h, libsnarkv_host.so): a
`host_api.Protocol` and the witness polynomials of a `Context` in device memory in, proof bytes out.

    with PlonkProver(protocol, ctx, d_srs, d_preprocessed, instances, mos, transcript) as p:
        challenges = p.phase(d_advice)                        # one call per entry of the protocol's num_witness
        challenges += p.phase(None)                           # a phase without witnesses
        challenges += p.phase(d_z, form=FORM_VALUES)          # made from the challenges so far
        proof = p.finish()                                    # None: the witness does not satisfy the constraints

`plan(protocol)` needs no device: what the protocol compiles to, or the refusal as a `HostError`.

`flags=QUOTIENT_COSETS` on `plan` and `PlonkProver` (include/snarkv_host_plonk_prove_opts.h): the session takes the quotient
one coset of the domain at a time, over a work region 2^e times smaller; the proof bytes are the same.

The ctypes tables are this module's own: one table per header."""
import ctypes

from . import host_api as H
from ._bind import Api, addr as _addr

_vp, _cp, _sz, _int = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
_szp = ctypes.POINTER(_sz)

MOS_GWC19, MOS_BDFG21 = 0, 1
TRANSCRIPT_EVM, TRANSCRIPT_POSEIDON = 0, 1
FORM_COEFFS, FORM_VALUES = 0, 1
UNSATISFIED = "the witness does not satisfy the protocol's constraints"
QUOTIENT_COSETS = 1  # SNARKV_HOST_PLONK_QUOTIENT_COSETS

PREFIX = "snarkv_host_plonk_prover_"
# every function include/snarkv_host_plonk_prove.h declares, without the prefix
SHAPES = {
    "plan": (_int, [_vp, ctypes.POINTER(ctypes.c_uint32), _szp, _szp, _szp, _szp]),
    "begin": (_int, [_vp, _int, _int, _vp, _vp, _vp, _cp, _sz, ctypes.POINTER(_vp)]),
    "phase": (_int, [_vp, _vp, _int, _vp, _sz, _szp]),
    "finish": (_int, [_vp, _vp, _sz, _szp]),
    "destroy": (None, [_vp]),
}
SIGNATURES = {PREFIX + n: s for n, s in SHAPES.items()}
# ... and include/snarkv_host_plonk_prove_opts.h
_u32 = ctypes.c_uint32
OPTS_SHAPES = {
    "plan_opts": (_int, [_vp, _u32, ctypes.POINTER(_u32), _szp, _szp, _szp, _szp]),
    "begin_opts": (_int, [_vp, _int, _int, _u32, _vp, _vp, _vp, _cp, _sz, ctypes.POINTER(_vp)]),
}
OPTS_SIGNATURES = {PREFIX + n: s for n, s in OPTS_SHAPES.items()}
_bound = _bound_opts = None


def api():
    """the functions of the header, bound once: `api().begin` is snarkv_host_plonk_prover_begin"""
    global _bound
    if _bound is None:
        _bound = Api(H.load_library(), PREFIX, SHAPES)  # AttributeError if the header and the library drift
    return _bound


def opts_api():
    """the functions of the options header, bound once"""
    global _bound_opts
    if _bound_opts is None:
        _bound_opts = Api(H.load_library(), PREFIX, OPTS_SHAPES)
    return _bound_opts


def _check(rc):
    if rc < 0:
        raise H.HostError(rc, last_error())
    return rc


def last_error():
    return (H.load_library().snarkv_host_last_error() or b"").decode(errors="replace")


def pack_instances(instances):
    """[[int]] -> one packed instance block"""
    out = len(instances).to_bytes(4, "little")
    for column in instances:
        out += len(column).to_bytes(4, "little") + b"".join(int(v).to_bytes(32, "little") for v in column)
    return out


def plan(protocol, flags=0):
    """-> {"e", "n_cols", "n_instr", "n_consts", "bytes"}; a protocol the prover refuses raises HostError naming the cause.
    `bytes` is what a session begun with the same `flags` allocates."""
    e, cols, instr, consts, nbytes = ctypes.c_uint32(0), _sz(0), _sz(0), _sz(0), _sz(0)
    outs = (ctypes.byref(e), ctypes.byref(cols), ctypes.byref(instr), ctypes.byref(consts), ctypes.byref(nbytes))
    _check(opts_api().plan_opts(protocol._h, flags, *outs) if flags else api().plan(protocol._h, *outs))
    return {"e": e.value, "n_cols": cols.value, "n_instr": instr.value, "n_consts": consts.value, "bytes": nbytes.value}


class PlonkProver:
    """A prover session.  `instances`: [[int]] or a packed block.  The SRS (n points) and whatever a phase is given stay the
    caller's; the session keeps its own copy of every polynomial."""

    def __init__(self, protocol, ctx, d_srs, d_preprocessed, instances, mos=MOS_GWC19, transcript=TRANSCRIPT_EVM, flags=0):
        self._a, self._h = api(), None
        inst = bytes(instances) if isinstance(instances, (bytes, bytearray)) else pack_instances(instances)
        h = _vp()
        rest = (ctx._h, _addr(d_srs), _addr(d_preprocessed), inst, len(inst), ctypes.byref(h))
        _check(opts_api().begin_opts(protocol._h, mos, transcript, flags, *rest) if flags
               else self._a.begin(protocol._h, mos, transcript, *rest))
        self._h, self._keep = h, (protocol, ctx, d_srs)

    def phase(self, d_witness, form=FORM_COEFFS):
        """the next phase's polynomials (None for a phase without any) -> the challenges squeezed after them, as ints"""
        n = _sz(0)
        out = ctypes.create_string_buffer(32 * 64)
        _check(self._a.phase(self._h, _addr(d_witness), form, out, 64, ctypes.byref(n)))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n.value)]

    def finish(self):
        """-> the proof bytes, or None when the witness does not satisfy the protocol's constraints"""
        n = _sz(0)
        rc = self._a.finish(self._h, None, 0, ctypes.byref(n))
        if rc != H.ERR_CAPACITY:
            _check(rc)
            return b"" if rc == 1 else None
        out = ctypes.create_string_buffer(n.value)
        rc = _check(self._a.finish(self._h, out, len(out), ctypes.byref(n)))
        return out.raw[:n.value] if rc == 1 else None

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
