"""The PLONK prover on pallas for protocols with committed instances (include/snarkv_host_pallas_plonk_prove_ci.h,
libsnarkv_host_pallas_plonk_prove_ci.so): `host_plonk_prove_pallas`'s session under the library's other entries, which accept
an `instance_committing_key` and queries of instance polynomials -- the shape of halo2's proofs over IPA.  `begin` commits the
instance columns (blind 1 over the key's `constant`, which must be the key's s) and hashes the points; the verifier recomputes
them over `bases`, which must be the first points of the key's Lagrange basis (`g1_ntt.dk_lagrange_dev`) and are not checked.

    with PlonkProver(protocol, ctx, dk, h, s, d_preprocessed, pre_blinds, instances) as p: ...   # as host_plonk_prove_pallas

The ctypes table is this module's own: one table per header."""
import ctypes
import os

from . import host_api_pallas as H
from . import host_plonk_prove_pallas as _B
from ._bind import Api
from .host_plonk_prove_pallas import FORM_COEFFS, FORM_VALUES, QUOTIENT_COSETS, UNSATISFIED, pack_instances  # noqa: F401

LIB_NAME = "libsnarkv_host_pallas_plonk_prove_ci.so"
PREFIX = "snarkv_host_pallas_plonk_ci_prover_"
# every function include/snarkv_host_pallas_plonk_prove_ci.h declares, without the prefix: the shapes of the other header's
SHAPES = dict(_B.SHAPES)
SIGNATURES = {PREFIX + n: s for n, s in SHAPES.items()}
_bound = None


def lib_path():
    return os.environ.get("SNARKV_HOST_PALLAS_PLONK_PROVE_CI_LIB") or os.path.join(H.HERE, LIB_NAME)


def api():
    """the functions of the header, bound once.  No fallback: a missing library raises."""
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


def plan(protocol, flags=0):
    """as host_plonk_prove_pallas.plan, a protocol with an instance_committing_key accepted"""
    _u32, _sz = ctypes.c_uint32, ctypes.c_size_t
    e, cols, instr, consts, nbytes = _u32(0), _sz(0), _sz(0), _sz(0), _sz(0)
    rc = api().plan(protocol._h, flags, ctypes.byref(e), ctypes.byref(cols), ctypes.byref(instr), ctypes.byref(consts), ctypes.byref(nbytes))
    if rc < 0:
        raise H.HostError(rc, last_error())
    return {"e": e.value, "n_cols": cols.value, "n_instr": instr.value, "n_consts": consts.value, "bytes": nbytes.value}


class PlonkProver(_B.PlonkProver):
    """`host_plonk_prove_pallas.PlonkProver` over this module's library"""

    _api = staticmethod(api)
