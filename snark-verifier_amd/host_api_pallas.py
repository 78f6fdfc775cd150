"""ctypes binding of include/snarkv_host_pallas.h -- the C API of the pasta flavour of the C++ host mirror
(libsnarkv_host_pallas.so): verify and aggregate halo2 IPA proofs on pallas.

Everything here moves bytes; the verifier logic is the C++ mirror of the reference's API and every EC operation runs on
the device behind it (libsnarkv_pallas.so).  `tests/test_host_pallas_capi_symbols.py` checks that `_SIGNATURES` and the
header agree."""
import ctypes
import os

from .host_api import (  # noqa: F401  (the codes are include/snarkv_host.h's)
    ERR_ARG,
    ERR_CAPACITY,
    ERR_DEVICE,
    ERR_INVALID_INSTANCES,
    ERR_INVALID_PROTOCOL,
    ERR_OTHER,
    ERR_PANIC,
    ERR_TRAILING,
    ERR_TRANSCRIPT,
    HostError,
    pack_proofs,
)

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libsnarkv_host_pallas.so"

DECOMPRESS_HOST, DECOMPRESS_DEVICE, DECOMPRESS_AUTO = 0, 1, 2
DEVICE_MIN = 1  # SNARKV_HOST_PALLAS_DEVICE_MIN

_vp, _cp, _sz, _u32, _int, _uint = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint
_pp = ctypes.POINTER(ctypes.c_void_p)
_psz = ctypes.POINTER(ctypes.c_size_t)
_pd = ctypes.POINTER(ctypes.c_double)

# name -> (restype, argtypes); every function include/snarkv_host_pallas.h declares
_SIGNATURES = {
    "snarkv_host_pallas_last_error": (_cp, []),
    "snarkv_host_pallas_protocol_parse": (_int, [_cp, _sz, _pp]),
    "snarkv_host_pallas_protocol_free": (None, [_vp]),
    "snarkv_host_pallas_ipa_dk_create": (_int, [_u32, _cp, _cp, _cp, _pp]),
    "snarkv_host_pallas_ipa_dk_free": (None, [_vp]),
    "snarkv_host_pallas_plonk_succinct_verify_batch": (_int, [_vp, _vp, _cp, _sz, _cp, _sz, _u32, _uint, _int, _vp, _sz]),
    "snarkv_host_pallas_ipa_decide_all": (_int, [_vp, _cp, _u32, _vp]),
    "snarkv_host_pallas_plonk_verify": (_int, [_vp, _vp, _cp, _sz, _cp, _sz, _u32, _uint, _int]),
    "snarkv_host_pallas_ipa_as_create_proof": (_int, [_vp, _cp, _u32, _cp, _sz, _vp, _sz, _psz, _vp]),
    "snarkv_host_pallas_ipa_as_verify": (_int, [_vp, _cp, _u32, _cp, _sz, _vp]),
    "snarkv_host_pallas_aggregate": (_int, [_vp, _vp, _cp, _sz, _cp, _sz, _u32, _uint, _int, _cp, _sz, _pd, _vp, _sz, _psz,
                                            _vp]),
}

# name -> (restype, argtypes); every function include/snarkv_host_pallas_fold.h declares (libsnarkv_host_pallas_fold.so: a
# library and a table of its own, as the header is)
_FOLD_LIB_NAME = "libsnarkv_host_pallas_fold.so"
_FOLD_SIGNATURES = {
    "snarkv_host_pallas_fold_last_error": (_cp, []),
    "snarkv_host_pallas_ipa_fold_challenge": (_int, [_vp, _cp, _u32, _cp, _vp]),
    "snarkv_host_pallas_ipa_decide_all_folded": (_int, [_vp, _cp, _u32, _cp, _vp]),
    "snarkv_host_pallas_plonk_verify_folded": (_int, [_vp, _vp, _cp, _sz, _cp, _sz, _u32, _uint, _int, _cp]),
}

# name -> (restype, argtypes); every function include/snarkv_host_pallas_prove.h declares (libsnarkv_host_pallas_prove.so)
_PROVE_LIB_NAME = "libsnarkv_host_pallas_prove.so"
_PROVE_SIGNATURES = {
    "snarkv_host_pallas_prove_last_error": (_cp, []),
    "snarkv_host_pallas_ipa_create_proof": (_int, [_vp, _cp, _sz, _cp, _cp, _cp, _cp, _cp, _sz, _vp, _sz, _psz, _vp]),
}

_lib = None
_fold_lib = None
_prove_lib = None


def lib_path():
    return os.environ.get("SNARKV_HOST_PALLAS_LIB") or os.path.join(HERE, _LIB_NAME)


def load_library():
    """Loads libsnarkv_host_pallas.so (which binds libsnarkv_pallas.so next to it).  No fallback: a missing library raises."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise HostError(ERR_DEVICE, "%s not built (run `python __graft_entry__.py`)" % path)
        from .pallas import load_library as _load_device_library

        _load_device_library()  # torch's HIP runtime and libsnarkv_pallas.so first, through their own loader
        L = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def fold_lib_path():
    return os.environ.get("SNARKV_HOST_PALLAS_FOLD_LIB") or os.path.join(HERE, _FOLD_LIB_NAME)


def load_fold_library():
    """Loads libsnarkv_host_pallas_fold.so (which binds libsnarkv_host_pallas.so and libsnarkv_pallas.so next to it)."""
    global _fold_lib
    if _fold_lib is None:
        path = fold_lib_path()
        if not os.path.exists(path):
            raise HostError(ERR_DEVICE, "%s not built (run `python __graft_entry__.py`)" % path)
        load_library()
        L = ctypes.CDLL(path)
        for name, (res, args) in _FOLD_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _fold_lib = L
    return _fold_lib


def prove_lib_path():
    return os.environ.get("SNARKV_HOST_PALLAS_PROVE_LIB") or os.path.join(HERE, _PROVE_LIB_NAME)


def load_prove_library():
    """Loads libsnarkv_host_pallas_prove.so (which binds libsnarkv_host_pallas.so and libsnarkv_pallas.so next to it)."""
    global _prove_lib
    if _prove_lib is None:
        path = prove_lib_path()
        if not os.path.exists(path):
            raise HostError(ERR_DEVICE, "%s not built (run `python __graft_entry__.py`)" % path)
        load_library()
        L = ctypes.CDLL(path)
        for name, (res, args) in _PROVE_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _prove_lib = L
    return _prove_lib


def _check_fold(rc):
    if rc < 0:
        raise HostError(rc, (load_fold_library().snarkv_host_pallas_fold_last_error() or b"").decode(errors="replace"))
    return rc


def _check(rc):
    """negative codes raise; 1 / 0 (accept / reject) pass through"""
    if rc < 0:
        raise HostError(rc, (load_library().snarkv_host_pallas_last_error() or b"").decode(errors="replace"))
    return rc


class _Handle:
    _free = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._free)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Protocol(_Handle):
    """A parsed `PlonkProtocol` (verifier/plonk/protocol.rs:19-71), from the packed form of host/wire.hpp."""
    _free = "snarkv_host_pallas_protocol_free"

    def __init__(self, data):
        self._L = load_library()
        h = ctypes.c_void_p()
        _check(self._L.snarkv_host_pallas_protocol_parse(bytes(data), len(data), ctypes.byref(h)))
        self._h = h


class IpaDecidingKey(_Handle):
    """`IpaDecidingKey` (pcs/ipa/decider.rs:3-22): g = 2^k points (64 B each), h, and S for a zero-knowledge key."""
    _free = "snarkv_host_pallas_ipa_dk_free"

    def __init__(self, k, g, h, s=None):
        self._L = load_library()
        assert len(g) == 64 << k and len(h) == 64 and (s is None or len(s) == 64)
        self.k, self.zk = k, s is not None
        hd = ctypes.c_void_p()
        _check(self._L.snarkv_host_pallas_ipa_dk_create(k, bytes(g), bytes(h), None if s is None else bytes(s), ctypes.byref(hd)))
        self._h = hd

    @property
    def acc_bytes(self):
        return 32 * self.k + 64


def plonk_succinct_verify_batch(protocol, dk, instances, proofs, n, host_threads=0, decompress=DECOMPRESS_AUTO):
    """N x PlonkSuccinctVerifier::{read_proof, verify}, the succinct-check MSMs in one device launch -> (code, the n
    accumulators concatenated or None): code 1 done, 0 a succinct check failed.  Malformed input raises `HostError`."""
    L = load_library()
    out = ctypes.create_string_buffer(max(1, dk.acc_bytes * n))
    rc = _check(L.snarkv_host_pallas_plonk_succinct_verify_batch(protocol._h, dk._h, instances, len(instances), proofs, len(proofs),
                                                                 n, host_threads, decompress, out, len(out)))
    return rc, (out.raw[: dk.acc_bytes * n] if rc == 1 else None)


def ipa_decide_all(dk, accs):
    """(all accepted, per-accumulator verdicts)"""
    m = len(accs) // dk.acc_bytes
    assert len(accs) == m * dk.acc_bytes
    ok = ctypes.create_string_buffer(max(1, m))
    rc = _check(load_library().snarkv_host_pallas_ipa_decide_all(dk._h, bytes(accs), m, ok))
    return rc == 1, [b != 0 for b in ok.raw[:m]]


def plonk_verify(protocol, dk, instances, proofs, n, host_threads=0, decompress=DECOMPRESS_AUTO):
    return _check(load_library().snarkv_host_pallas_plonk_verify(protocol._h, dk._h, instances, len(instances), proofs, len(proofs),
                                                                 n, host_threads, decompress)) == 1


def _seed(seed):
    assert seed is None or len(seed) == 32
    return None if seed is None else bytes(seed)


def ipa_fold_challenge(dk, accs, seed=None):
    """rho of the folded decide: BLAKE2b-512 (personalisation `snarkv_ipa_fold1`) over `u32le k | u32le m | accs | seed`,
    reduced mod r as the Blake2b transcript squeezes -> 32 bytes LE.  No device work."""
    m = len(accs) // dk.acc_bytes
    assert len(accs) == m * dk.acc_bytes
    rho = ctypes.create_string_buffer(32)
    _check_fold(load_fold_library().snarkv_host_pallas_ipa_fold_challenge(dk._h, bytes(accs), m, _seed(seed), rho))
    return rho.raw


def ipa_decide_all_folded(dk, accs, seed=None, verdicts=True):
    """`decide_all` as one folded check with rho derived from the accumulators -> (all accepted, per-accumulator verdicts
    or None).  With `verdicts` a rejected batch is decided again one by one to name the culprits."""
    m = len(accs) // dk.acc_bytes
    assert len(accs) == m * dk.acc_bytes
    ok = ctypes.create_string_buffer(max(1, m)) if verdicts else None
    rc = _check_fold(load_fold_library().snarkv_host_pallas_ipa_decide_all_folded(dk._h, bytes(accs), m, _seed(seed), ok))
    return rc == 1, ([b != 0 for b in ok.raw[:m]] if verdicts else None)


def plonk_verify_folded(protocol, dk, instances, proofs, n, host_threads=0, decompress=DECOMPRESS_AUTO, seed=None):
    """`plonk_verify` with the folded decide as its second half"""
    return _check_fold(load_fold_library().snarkv_host_pallas_plonk_verify_folded(
        protocol._h, dk._h, instances, len(instances), proofs, len(proofs), n, host_threads, decompress, _seed(seed))) == 1


def ipa_create_proof(dk, poly, z, omega=None, p_bar=None, omega_bar=None, absorbed=b""):
    """`Ipa::create_proof` in one call, halo2's Blake2b transcript on the device -> (proof bytes, accumulator bytes).
    `poly` (and `p_bar`) = 2^k scalars packed 32 bytes each, `z`, `omega`, `omega_bar` 32 bytes; a zero-knowledge key
    takes omega, p_bar and omega_bar, any other key none of them.  `absorbed`: what the transcript's hasher took so far."""
    L = load_prove_library()
    cap = 64 * dk.k + 128
    proof, ln, acc = ctypes.create_string_buffer(cap), ctypes.c_size_t(0), ctypes.create_string_buffer(dk.acc_bytes)
    opt = lambda v: None if v is None else bytes(v)  # noqa: E731
    rc = L.snarkv_host_pallas_ipa_create_proof(dk._h, bytes(poly), len(poly) // 32, bytes(z), opt(omega), opt(p_bar),
                                               opt(omega_bar), bytes(absorbed) or None, len(absorbed), proof, cap,
                                               ctypes.byref(ln), acc)
    if rc < 0:
        raise HostError(rc, (L.snarkv_host_pallas_prove_last_error() or b"").decode(errors="replace"))
    return proof.raw[:ln.value], acc.raw


def _as_proof_cap(dk):
    return 32 * (2 * dk.k + 8) + 64


def ipa_as_create_proof(dk, accs, rand=b""):
    """`IpaAs::create_proof` (accumulation.rs:148-226) over a fresh Blake2b transcript; `rand`: the 32-byte scalars the
    reference would draw, concatenated -> (accumulator, accumulation proof)"""
    m = len(accs) // dk.acc_bytes
    acc, proof, n = ctypes.create_string_buffer(dk.acc_bytes), ctypes.create_string_buffer(_as_proof_cap(dk)), ctypes.c_size_t(0)
    _check(load_library().snarkv_host_pallas_ipa_as_create_proof(dk._h, bytes(accs), m, bytes(rand), len(rand) // 32, proof, len(proof),
                                                                 ctypes.byref(n), acc))
    return acc.raw, proof.raw[: n.value]


def ipa_as_verify(dk, accs, proof):
    """`IpaAs::{read_proof, verify}` (accumulation.rs:21-146) -> (code, accumulator or None)"""
    m = len(accs) // dk.acc_bytes
    acc = ctypes.create_string_buffer(dk.acc_bytes)
    rc = _check(load_library().snarkv_host_pallas_ipa_as_verify(dk._h, bytes(accs), m, bytes(proof), len(proof), acc))
    return rc, (acc.raw if rc == 1 else None)


def aggregate(protocol, dk, instances, proofs, n, rand=b"", host_threads=0, decompress=DECOMPRESS_AUTO, timings=False):
    """succinct-verify n proofs, accumulate, decide -> (accepted, accumulator, accumulation proof[, timings dict])"""
    L = load_library()
    tm = (ctypes.c_double * 5)()
    acc, proof, ln = ctypes.create_string_buffer(dk.acc_bytes), ctypes.create_string_buffer(_as_proof_cap(dk)), ctypes.c_size_t(0)
    rc = _check(L.snarkv_host_pallas_aggregate(protocol._h, dk._h, instances, len(instances), proofs, len(proofs), n, host_threads,
                                               decompress, bytes(rand), len(rand) // 32, tm, proof, len(proof), ctypes.byref(ln), acc))
    out = (rc == 1, acc.raw, proof.raw[: ln.value])
    if timings:
        return out + (dict(zip(("read_proofs", "succinct_verify", "accumulate", "decide", "total"), list(tm))),)
    return out
