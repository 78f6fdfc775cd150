"""Child process of tests/test_gpu_ipa_create.py: the one-call IPA proof of the pallas product API
(`host_api_pallas.ipa_create_proof`, include/snarkv_host_pallas_prove.h) at k = 3 and k = 8 against the device ABI
(`ipa_create.create_proof` on a context of its own), its accumulator through `ipa_decide_all`, and a zero-knowledge key at
k = 3.  Prints `k3_equal=... k3_decides=... k8_equal=... k8_decides=... zk_equal=...`."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import pallas as PA  # noqa: E402


def one(pctx, k, zk):
    from snark_verifier_amd import host_api_pallas as H
    from snark_verifier_amd import ipa_create as CR

    n = 1 << k
    base = PA.sample_points(80 + k, 34)
    rnd = random.Random("product-%d-%d" % (k, zk))
    fe = lambda: PA.fe_to_bytes(rnd.randrange(PA.R))  # noqa: E731
    # n + 2 points as two-term combinations of a few sampled ones, in one segmented launch
    sc = b"".join(PA.fe_to_bytes(rnd.randrange(1, PA.R)) for _ in range(2 * (n + 2)))
    pts = b"".join(PA.g1_to_bytes(base[rnd.randrange(34)]) + PA.g1_to_bytes(base[rnd.randrange(34)]) for _ in range(n + 2))
    gb = pctx.msm_batched(sc, pts, [2 * i for i in range(n + 3)])
    g, h, s = gb[:64 * n], gb[64 * n:64 * n + 64], (gb[64 * n + 64:] if zk else None)
    poly, z = b"".join(fe() for _ in range(n)), fe()
    omega, p_bar, omega_bar = (fe(), b"".join(fe() for _ in range(n)), fe()) if zk else (None, None, None)
    pre = rnd.randbytes(77)
    hdk = H.IpaDecidingKey(k, g, h, s)
    proof, acc = H.ipa_create_proof(hdk, poly, z, omega, p_bar, omega_bar, pre)
    ddk = pctx.ipa_dk_create(g)
    want_proof, (xi, u) = CR.create_proof(pctx, ddk, h, s, poly, z, omega, p_bar, omega_bar, pre)
    want_acc = b"".join(PA.fe_to_bytes(x) for x in xi) + PA.fe_to_bytes(u[0]) + PA.fe_to_bytes(u[1])
    equal = proof == want_proof and acc == want_acc and len(proof) == 64 * k + 64 + (64 if zk else 0)
    decides = H.ipa_decide_all(hdk, acc) == (True, [True])
    ddk.close()
    hdk.close()
    return equal, decides


def main():
    from snark_verifier_amd import host_api_pallas as H
    from snark_verifier_amd import pallas as PL

    H.load_prove_library()
    pctx = PL.PallasContext(0)
    e3, d3 = one(pctx, 3, False)
    e8, d8 = one(pctx, 8, False)
    ez, dz = one(pctx, 3, True)
    pctx.close()
    print("k3_equal=%s k3_decides=%s k8_equal=%s k8_decides=%s zk_equal=%s" % (e3, d3, e8, d8, ez and dz))


if __name__ == "__main__":
    main()
