"""Child process of tests/test_gpu_ipa_batch.py: `host_api_pallas.plonk_verify` on the forged k = 8 proofs of the file
given, under whatever SNARKV_IPA_SHARED the parent set (the knob is read once per process).  `--forge FILE` writes the
file instead (pure Python).  Prints `accept=... reject=...`."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, N = 8, 4


def forge(path):
    import hostfmt
    import pallas as PA
    import plonk as P
    import plonk_synth as S
    import transcript as T

    S.use_curve(PA)
    hostfmt.use_curve(PA)
    rng = random.Random("ipa-batch-product")
    pr, dl = S.standard_plonk_protocol(rng, k=K, num_instance=(3,))
    kd = {"g": [rng.randrange(1, PA.R) for _ in range(1 << K)], "h": rng.randrange(1, PA.R), "s": rng.randrange(1, PA.R)}
    mk = lambda stream=b"": T.Blake2bTranscript(PA, stream)  # noqa: E731
    insts = [[[rng.randrange(PA.R) for _ in range(3)]] for _ in range(N)]
    d = {"protocol": S.pack_protocol(pr), "g": b"".join(PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, c)) for c in kd["g"]),
         "h": PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, kd["h"])), "s": PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, kd["s"])),
         "instances": [S.pack_instances(x) for x in insts],
         "proofs": [P.forge_proof_ipa(pr, insts[i], kd, mk, rng, dl) for i in range(N)]}
    with open(path, "w") as f:
        json.dump({k: v.hex() if isinstance(v, bytes) else [x.hex() for x in v] for k, v in d.items()}, f)


def main():
    if sys.argv[1] == "--forge":
        return forge(sys.argv[2])
    from snark_verifier_amd import host_api_pallas as H

    with open(sys.argv[1]) as f:
        d = {k: bytes.fromhex(v) if isinstance(v, str) else [bytes.fromhex(x) for x in v] for k, v in json.load(f).items()}
    H.load_library()
    protocol = H.Protocol(d["protocol"])
    dk = H.IpaDecidingKey(K, d["g"], d["h"], d["s"])
    ib, proofs = b"".join(d["instances"]), d["proofs"]
    accept = bool(H.plonk_verify(protocol, dk, ib, H.pack_proofs(proofs), N))
    # U is the last point of a proof, followed by the scalar c (pcs/ipa.rs:121-122): another proof's U there is a valid
    # encoding, so the proof still reads, and what it then claims no longer holds
    bad = list(proofs)
    p = bytearray(bad[N // 2])
    assert bad[0][-64:-32] != bytes(p[-64:-32])
    p[-64:-32] = bad[0][-64:-32]
    bad[N // 2] = bytes(p)
    try:
        reject = not H.plonk_verify(protocol, dk, ib, H.pack_proofs(bad), N)
    except Exception:
        reject = True
    print("accept=%s reject=%s" % (accept, reject))


if __name__ == "__main__":
    main()
