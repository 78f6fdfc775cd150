"""MI355X-native KZG accumulation hot path (after privacy-scaling-explorations/snark-verifier).

Thin Python binding over the C ABI in `include/snarkv_amd.h` (ctypes).  The
product is `libsnarkv_amd.so` -- hand-written HIP kernels for gfx950 -- and the
C++ host mirror in `host/`; Python only moves bytes and device pointers and
provides `torch.distributed` plumbing for the multi-GPU fold.

There is NO CPU fallback: importing works anywhere, but creating a `Context`
without the built library or without a HIP device raises.
"""
# HIP multiplexes a process's streams onto a fixed number of hardware queues (the runtime's default is 4) and kernels of
# streams that share a queue run one after the other.  The queue count is the runtime's and the host's setting: neither
# the package nor the library changes it (csrc/ctx.hip).

from ._lib import (  # noqa: F401
    Context,
    DecidingKey,
    IpaDecidingKey,
    MultiGpu,
    PoseidonSpec,
    SnarkvError,
    last_error,
    lib_path,
    load_library,
    SNARKV_FLAG_VALIDATE,
    SNARKV_FLAG_MONTGOMERY,
    SNARKV_HOST_BUFFERS,
    SNARKV_ERR_EMPTY,
    SNARKV_ERR_LENGTH,
    SNARKV_ERR_ENCODING,
    SNARKV_ERR_DEVICE,
    SNARKV_ERR_ARG,
    PIP_STAGE_NAMES,
    G1_PARTIAL_BYTES,
)

from . import host_api  # noqa: F401,E402  (C API of the C++ host mirror: include/snarkv_host.h)
from . import host_api_pallas  # noqa: F401,E402  (the pasta flavour of the host mirror: include/snarkv_host_pallas.h)
from . import ipa_prover  # noqa: F401,E402  (the IPA prover on the device: include/snarkv_ipa_prover.h)
from .ipa_prover import IpaProver  # noqa: F401,E402
from . import ipa_batch  # noqa: F401,E402  (many vectors against one resident IPA key: include/snarkv_ipa_batch.h)
from . import ipa_commit_blinded  # noqa: F401,E402  (many blinded commitments per call: include/snarkv_ipa_commit_blinded.h)
from . import ipa_fold  # noqa: F401,E402  (decide_all as one folded check: include/snarkv_ipa_fold.h)
from . import ipa_create  # noqa: F401,E402  (Ipa::create_proof in one call, Blake2b transcript on the device: include/snarkv_ipa_create.h)
from . import poly  # noqa: F401,E402  (resident polynomials: linear combination, evaluation, division: include/snarkv_poly.h)
from . import ntt  # noqa: F401,E402  (forward, inverse and coset transforms of resident polynomials: include/snarkv_ntt.h)
from . import g1_ntt  # noqa: F401,E402  (the transform over group elements, a key's Lagrange basis: include/snarkv_g1_ntt.h)
from . import poly_prod  # noqa: F401,E402  (column products: batch inversion, grand product, permutation Z: include/snarkv_poly_prod.h)
from . import quotient  # noqa: F401,E402  (the quotient on the extended coset: extension, gate program, vanishing division: include/snarkv_quotient.h)
from . import lookup  # noqa: F401,E402  (the lookup argument: sort, permuted columns, product Z: include/snarkv_lookup.h)
from . import ipa_multiopen  # noqa: F401,E402  (the Bgh19 multi-open prover in one call: include/snarkv_ipa_multiopen.h)
from . import poly_batch  # noqa: F401,E402  (many evaluations of resident polynomials in one call: include/snarkv_poly_batch.h)
from . import kzg_multiopen  # noqa: F401,E402  (the Gwc19 and Bdfg21 multi-open provers, BN254: include/snarkv_kzg_multiopen.h)
from . import host_kzg_open  # noqa: F401,E402  (the same through the host mirror and its transcripts: include/snarkv_host_kzg_open.h)
from . import host_plonk_prove  # noqa: F401,E402  (the PLONK prover session of the host mirror: include/snarkv_host_plonk_prove.h)
from . import host_plonk_prove_pallas_ci  # noqa: F401,E402  (... with committed instances: include/snarkv_host_pallas_plonk_prove_ci.h)
from . import host_plonk_prove_pallas  # noqa: F401,E402  (... on pallas over IPA: include/snarkv_host_pallas_plonk_prove.h)

__all__ = [
    "host_api",
    "host_api_pallas",
    "ipa_prover",
    "ipa_batch",
    "ipa_commit_blinded",
    "ipa_fold",
    "ipa_create",
    "poly",
    "ntt",
    "g1_ntt",
    "poly_prod",
    "quotient",
    "lookup",
    "ipa_multiopen",
    "poly_batch",
    "kzg_multiopen",
    "host_kzg_open",
    "host_plonk_prove",
    "host_plonk_prove_pallas",
    "host_plonk_prove_pallas_ci",
    "IpaProver",
    "Context",
    "DecidingKey",
    "IpaDecidingKey",
    "MultiGpu",
    "PoseidonSpec",
    "SnarkvError",
    "last_error",
    "lib_path",
    "load_library",
    "SNARKV_FLAG_VALIDATE",
    "SNARKV_FLAG_MONTGOMERY",
    "SNARKV_HOST_BUFFERS",
    "SNARKV_ERR_EMPTY",
    "SNARKV_ERR_LENGTH",
    "SNARKV_ERR_ENCODING",
    "SNARKV_ERR_DEVICE",
    "SNARKV_ERR_ARG",
    "PIP_STAGE_NAMES",
    "G1_PARTIAL_BYTES",
]
