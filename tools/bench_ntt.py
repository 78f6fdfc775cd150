"""Times the transform (snark_verifier_amd.ntt.ntt_dev / intt_dev, polynomials resident on the device) on BN254 and pallas at
k = 10, 16, 20, 24 with count = 1 and 17, forward and inverse, next to two yardsticks taken in the same process:

  (a) one commitment of a 2^k vector over the resident key (`ipa_commit_batch_dev`, m = 1): the operation a transform sits
      beside in a prover;
  (b) a device-to-device copy of count * 2^k * 32 bytes, times the number of passes of the transform: what moving the data
      once per pass costs, the memory floor of the pass structure.

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise).

    python tools/bench_ntt.py [--ks 10,16,20,24] [--counts 1,17] [--curves bn254,pallas] [--out FILE]

`/commit` is the transform's time per polynomial over one commitment, `/copy` its time over the copies.  The last column says
which of the two it is closer to (in the logarithm): "copy" means the memory floor is the yardstick that tells something about
the result, "commit" that a transform is as dear as the commitment next to it.  Nothing routes on these numbers."""
import argparse
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ipa_create import pallas_points  # noqa: E402
from bench_ipa_multiopen import device_scalars  # noqa: E402

WARMUPS, RUNS = 3, 11


def timed(fn, sync):
    ts = []
    for i in range(WARMUPS + RUNS):
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= WARMUPS:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%9.3f [%9.3f .. %9.3f]" % t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20,24")
    ap.add_argument("--counts", default="1,17")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_batch as IB
    from snark_verifier_amd import ntt as N
    from snark_verifier_amd import pallas as PL

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max]" % (RUNS, WARMUPS),
             "# commit: ipa_commit_batch_dev of one 2^k vector over the resident key; copy: device-to-device copy of the data x passes",
             "# curve   k  count dir passes   transform                          commit (m = 1)                     copy x passes"
             "                      /commit   /copy  nearer",
             "# /commit: transform per polynomial (time / count) over one commitment; /copy: transform over the copies"]
    counts = [int(x) for x in a.counts.split(",")]
    for curve in a.curves.split(","):
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        for k in [int(x) for x in a.ks.split(",")]:
            n = 1 << k
            rnd = random.Random("bench-ntt-%s-%d" % (curve, k))
            if curve == "bn254":
                d = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
                ctx.sample_points_dev(k, n, d.data_ptr())
                ctx.sync()
                dk = sv.IpaDecidingKey(ctx, d.cpu().numpy().tobytes())
                del d
            else:
                dk = ctx.ipa_dk_create(pallas_points(ctx, rnd, n))
            d_in = device_scalars(torch, max(counts) * n, 3000 + k)
            d_out = torch.empty_like(d_in)
            d_com = torch.empty(64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t_commit = timed(lambda: IB.commit_batch_dev(ctx, dk, d_in.data_ptr(), n, 1, d_com.data_ptr()), ctx.sync)
            for count in counts:
                size = 32 * n * count
                passes = N.passes(k)
                t_once = timed(lambda: d_out[:size].copy_(d_in[:size]), torch.cuda.synchronize)
                t_copy = tuple(passes * t for t in t_once)
                for name, fn in (("fwd", N.ntt_dev), ("inv", N.intt_dev)):
                    t = timed(lambda: fn(ctx, d_in, d_out, k, count=count), ctx.sync)
                    per_commit, per_copy = t[0] / count / t_commit[0], t[0] / t_copy[0]
                    nearer = "copy" if abs(math.log(per_copy)) < abs(math.log(per_commit)) else "commit"
                    lines.append("%-7s %3d %5d %s %5d   %s   %s   %s   %7.2f %7.2f  %s" % (
                        curve, k, count, name, passes, fmt(t), fmt(t_commit), fmt(t_copy), per_commit, per_copy, nearer))
                    print(lines[-1], flush=True)
            dk.close()
            del d_in, d_out
        ctx.close()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
