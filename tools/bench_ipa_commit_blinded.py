"""Times snarkv_ipa_commit_blinded_batch_dev (include/snarkv_ipa_commit_blinded.h) on both curves at
(n, m) = (2^10, 8), (2^16, 8), (2^16, 1), next to two yardsticks of the same shape:

  plain        snarkv_ipa_commit_batch_dev: the same commitments without the blind term
  composed     (BN254 only: the pasta build has no device-resident segmented MSM in its public interface)
               snarkv_ipa_commit_batch_dev, then ONE segmented launch of m 2-term MSMs [1, blind_a] x [C_a, S] through
               snarkv_g1_msm_batched_dev -- the blind step of ipa_enqueue_commit (csrc/ipa_prover.hip), for all vectors at
               once.  The pairs [C_a, S] are staged beforehand with the commitments of a first call: copying C_a into them is
               not timed, and the time of the launch does not depend on the values.

Every call is timed on the host clock up to the end of a synchronisation of the context's stream.  The key's window table is
built and the rows of S are with the context before anything is timed; scalars and blinds are random.  The three alternate in
one process: 3 warm-ups, then the median of 11 with [min .. max].

    python tools/bench_ipa_commit_blinded.py [--out profiles/ipa_commit_blinded_bench.txt]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUPS, RUNS = 3, 11
SHAPES = ((10, 8), (16, 8), (16, 1))
R = {"bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
     "pallas": 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001}
GEN = {"bn254": (1).to_bytes(32, "little") + (2).to_bytes(32, "little"),
       "pallas": ((1 << 254) + 45560315531419706090280762371685220353 - 1).to_bytes(32, "little") + (2).to_bytes(32, "little")}


def main():
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_commit_blinded as CB
    from snark_verifier_amd import pallas as PL

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# ms on the host clock, call + synchronisation: median of %d after %d warm-ups [min .. max]; the calls alternate" % (RUNS, WARMUPS),
             "# blinded: commit_blinded_batch_dev; plain: commit_batch_dev; composed: commit_batch_dev + one segmented launch of m 2-term MSMs",
             "# curve    n      m   blinded                        plain                          composed                       /plain  /composed"]

    def dev(raw):
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    for curve in ("bn254", "pallas"):
        rnd = random.Random("commit-blinded-" + curve)
        r = R[curve]
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        s64 = ctx.msm_batched(rnd.randrange(1, r).to_bytes(32, "little"), GEN[curve], [0, 1])
        for k, m in SHAPES:
            n = 1 << k
            # 2^k points s_i G: one segmented launch of single-term MSMs (no host curve arithmetic)
            sc = b"".join(rnd.randrange(1, r).to_bytes(32, "little") for _ in range(n))
            gb = ctx.msm_batched(sc, GEN[curve] * n, list(range(n + 1)))
            dk = sv.IpaDecidingKey(ctx, gb) if curve == "bn254" else ctx.ipa_dk_create(gb)
            dk.prepare()
            d_polys = torch.zeros(32 * n * m, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(64 * m, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if curve == "bn254":
                ctx.sample_scalars_dev(77, n * m, d_polys.data_ptr())
                ctx.sync()
            else:
                d_polys.copy_(dev(b"".join(rnd.randrange(r).to_bytes(32, "little") for _ in range(n * m))))
                torch.cuda.synchronize()
            blinds = [rnd.randrange(r) for _ in range(m)]
            bl = b"".join(b.to_bytes(32, "little") for b in blinds)

            def blinded():
                CB.commit_blinded_batch_dev(ctx, dk, s64, d_polys, n, m, bl, d_out)
                ctx.sync()

            def plain():
                ctx.ipa_commit_batch_dev(dk, d_polys.data_ptr(), n, m, d_out.data_ptr(), 0)
                ctx.sync()

            blinded()
            want = bytes(d_out.cpu().numpy())
            composed = None
            if curve == "bn254":
                plain()
                cs = bytes(d_out.cpu().numpy())
                d_pairs = dev(b"".join(cs[64 * a:64 * a + 64] + s64 for a in range(m)))
                d_sc = dev(b"".join((1).to_bytes(32, "little") + blinds[a].to_bytes(32, "little") for a in range(m)))
                d_off = torch.tensor([2 * a for a in range(m + 1)], dtype=torch.int32, device="cuda")
                d_out2 = torch.zeros(64 * m, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()

                def composed():
                    ctx.ipa_commit_batch_dev(dk, d_polys.data_ptr(), n, m, d_out.data_ptr(), 0)
                    ctx.msm_batched_dev(d_sc.data_ptr(), d_pairs.data_ptr(), d_off.data_ptr(), m, 2 * m, d_out2.data_ptr())
                    ctx.sync()

                composed()
                assert bytes(d_out2.cpu().numpy()) == want, "the composition and the blinded call disagree"
            calls = [blinded, plain] + ([composed] if composed else [])
            ts = [[] for _ in calls]
            for it in range(WARMUPS + RUNS):
                for i, f in enumerate(calls):
                    t0 = time.perf_counter()
                    f()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if it >= WARMUPS:
                        ts[i].append(dt)
            med = [statistics.median(t) for t in ts]
            cell = lambda t: "%8.3f [%8.3f .. %8.3f]" % (statistics.median(t), min(t), max(t))  # noqa: E731
            lines.append("  %-6s  %6d  %2d  %s  %s  %s  %6.2f  %s"
                         % (curve, n, m, cell(ts[0]), cell(ts[1]), cell(ts[2]) if composed else "%-29s" % "-",
                            med[0] / med[1], "%6.2f" % (med[0] / med[2]) if composed else "     -"))
            print(lines[-1], flush=True)
            dk.close()
            del d_polys, d_out
        ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
