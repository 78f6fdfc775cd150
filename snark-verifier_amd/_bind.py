"""What the ctypes modules of the IPA headers (`ipa_prover`, `ipa_batch`, `ipa_fold`, `ipa_create`, `ipa_multiopen`) and of
the resident-polynomial headers (`poly`, `ntt`, `poly_prod`, `quotient`, `lookup`) share: the binder of a module's own tables
to a library, the argument encoders, and the output buffers of the one-call provers.
The tables stay with their modules, one per header; this module knows no function name.
"""
import ctypes

from ._lib import SnarkvError, _as_bytes


class Api:
    """The functions of one table in one library: `api.name` is the library's `prefix + name`."""

    def __init__(self, lib, prefix, shapes, context_free=None):
        """`shapes`: name without the prefix -> (restype, argtypes).  `context_free`: attribute -> table of the forms on the
        default context, `bn254_...` and `pallas_...`; the library's own is bound and attached under the attribute."""
        self.lib, self.prefix = lib, prefix
        for n, (res, args) in shapes.items():
            fn = getattr(lib, prefix + n)  # AttributeError if the header and the library drift
            fn.restype, fn.argtypes = res, args
        curve = "pallas_" if prefix == "snarkv_pallas_" else "bn254_"
        for attr, table in (context_free or {}).items():
            name, = [n for n in table if n.startswith(curve)]
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = table[name]
            setattr(self, attr, fn)

    def __getattr__(self, name):
        return getattr(self.lib, self.prefix + name)

    def last_error(self):
        return (getattr(self.lib, self.prefix + "last_error")() or b"").decode(errors="replace")

    def check(self, rc):
        if rc < 0:
            raise SnarkvError(rc, self.last_error())
        return rc


_BOUND = {}


def _load_library(pallas):
    if pallas:
        from .pallas import load_library
    else:
        from ._lib import load_library
    return load_library()


def bind(shapes, context_free, pallas):
    """the `Api` of a module's tables in one library (`pallas`: the pasta build), bound once"""
    key = (id(shapes), bool(pallas))
    if key not in _BOUND:
        _BOUND[key] = Api(_load_library(pallas), "snarkv_pallas_" if pallas else "snarkv_", shapes, context_free)
    return _BOUND[key]


def is_pallas(ctx):
    from .pallas import PallasContext

    return isinstance(ctx, PallasContext)


def fe(v):
    """a scalar: an int or 32 bytes, None stays None"""
    return None if v is None else (int(v).to_bytes(32, "little") if isinstance(v, int) else _as_bytes(v))


def pt(p):
    """a point: an (x, y) int pair or 64 bytes, None stays None"""
    if p is None or isinstance(p, (bytes, bytearray)):
        return p
    return fe(int(p[0])) + fe(int(p[1]))


def vec(v):
    """a vector: a list of ints or packed bytes, None stays None"""
    if v is None or isinstance(v, (bytes, bytearray)):
        return v
    return b"".join(fe(int(c)) for c in v)


def addr(p):
    """a device address: an int or anything with `data_ptr()`, None stays None"""
    if p is None:
        return None
    return ctypes.c_void_p(int(p.data_ptr() if hasattr(p, "data_ptr") else p))


def u32s(idx):
    """an index array; an empty list still gives an address"""
    return (ctypes.c_uint32 * max(len(idx), 1))(*idx)


def scalars(vals):
    """scalars back to back; an empty list still gives an address"""
    return b"".join(fe(v) for v in vals) or b"\x00"


def signatures(shapes):
    """a module's table under the names of both libraries"""
    return {p + n: s for p in ("snarkv_", "snarkv_pallas_") for n, s in shapes.items()}


def prove(a, fn, k, cap, *args):
    """one call of a prover whose arguments end in (proof_out, proof_cap, proof_len, xi_out, u_out), with room for `cap`
    proof bytes -> (proof bytes, (xi, U))"""
    proof, plen = ctypes.create_string_buffer(cap), ctypes.c_size_t(0)
    xi, u = ctypes.create_string_buffer(32 * max(k, 1)), ctypes.create_string_buffer(64)
    a.check(fn(*args, proof, cap, ctypes.byref(plen), xi, u))
    xis = [int.from_bytes(xi.raw[32 * i:32 * i + 32], "little") for i in range(k)]
    return proof.raw[:plen.value], (xis, (int.from_bytes(u.raw[:32], "little"), int.from_bytes(u.raw[32:], "little")))
