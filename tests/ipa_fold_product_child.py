"""Child process of tests/test_gpu_ipa_fold.py: the folded decide of the pallas product API (`host_api_pallas.
ipa_decide_all_folded`, `plonk_verify_folded`) on the forged k = 8 proofs of the file given.  `--forge FILE` writes the file
instead (pure Python, as tests/ipa_batch_product_child.py forges its own).  Prints
`folded_accept=... folded_reject=... culprit=... plonk_equal=...`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ipa_batch_product_child as B  # noqa: E402

K, N = B.K, B.N


def main():
    if sys.argv[1] == "--forge":
        return B.forge(sys.argv[2])
    import hashlib

    from snark_verifier_amd import host_api_pallas as H

    with open(sys.argv[1]) as f:
        d = {k: bytes.fromhex(v) if isinstance(v, str) else [bytes.fromhex(x) for x in v] for k, v in json.load(f).items()}
    H.load_library()
    protocol = H.Protocol(d["protocol"])
    dk = H.IpaDecidingKey(K, d["g"], d["h"], d["s"])
    ib, pb = b"".join(d["instances"]), H.pack_proofs(d["proofs"])
    rc, accs = H.plonk_succinct_verify_batch(protocol, dk, ib, pb, N)
    assert rc == 1 and len(accs) == N * dk.acc_bytes
    seed = hashlib.sha256(b"ipa-fold-product").digest()
    accept = H.ipa_decide_all_folded(dk, accs) == (True, [True] * N)
    accept = accept and H.ipa_decide_all_folded(dk, accs, seed) == (True, [True] * N)
    accept = accept and H.ipa_decide_all_folded(dk, accs, seed, verdicts=False) == (True, None)
    accept = accept and H.ipa_decide_all_folded(dk, b"") == (True, [])  # decide_all of nothing
    # one accumulator's u swapped for another's
    stride, pos = dk.acc_bytes, N // 2
    u = lambda a: accs[a * stride + 32 * K:(a + 1) * stride]  # noqa: E731
    assert u(0) != u(pos)
    bad = accs[:pos * stride + 32 * K] + u(0) + accs[(pos + 1) * stride:]
    all_ok, verdicts = H.ipa_decide_all_folded(dk, bad, seed)
    reject = not all_ok and H.ipa_decide_all_folded(dk, bad, seed, verdicts=False) == (False, None)
    culprit = verdicts == [a != pos for a in range(N)] and H.ipa_decide_all(dk, bad) == (False, verdicts)
    plonk = H.plonk_verify(protocol, dk, ib, pb, N)
    plonk_equal = plonk is True and H.plonk_verify_folded(protocol, dk, ib, pb, N) == plonk \
        and H.plonk_verify_folded(protocol, dk, ib, pb, N, seed=seed) == plonk
    print("folded_accept=%s folded_reject=%s culprit=%s plonk_equal=%s" % (accept, reject, culprit, plonk_equal))


if __name__ == "__main__":
    main()
