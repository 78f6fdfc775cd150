"""Times the Bgh19 multi-open prover (snark_verifier_amd.ipa_multiopen.create_proof_dev, polynomials resident on the device)
next to the opening it ends in (snark_verifier_amd.ipa_create.create_proof_dev, zero-knowledge, one polynomial), alternating
in one process, on BN254 and pallas at k = 10, 16, 20: 3 warm-ups, then the median of 11 with [min .. max], ms per proof on
the host clock.

    python tools/bench_ipa_multiopen.py [--ks 10,16,20] [--curves bn254,pallas] [--out FILE]

The query shape is that of a StandardPlonk proof: 17 polynomials, all opened at x, the two
permutation products also at omega x and the first of them also at omega^last x -- three query sets of 15, 1 and 1
polynomials with 1, 2 and 3 points.  The evaluations come from `poly.eval_dev`.  The difference of the two columns is what
the multi-open front (4 linear combinations over 17 + 3 + 4 polynomials, 6 divisions, 4 evaluations, one more commitment)
adds to the opening.  Nothing routes on these numbers."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ipa_create import pallas_points, scalars  # noqa: E402

WARMUPS, RUNS = 3, 11
N_POLYS = 17


def device_scalars(torch, count, seed):
    """count canonical scalars on the device: 252 random bits each"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda", generator=g)
    t[:, 31] &= 0x0F
    return t.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import ipa_create as CR
    from snark_verifier_amd import ipa_multiopen as MO
    from snark_verifier_amd import pallas as PL
    from snark_verifier_amd import poly as P

    import bn254 as BN
    import pallas as PA

    field = {"bn254": BN.R, "pallas": PA.R}
    lines = ["# ms per proof on the host clock: median of %d after %d warm-ups [min .. max]; the two calls alternate" % (RUNS, WARMUPS),
             "# multi-open: %d polynomials on the device, 3 query sets (15 | 1 | 1 polynomials at 1 | 2 | 3 points)" % N_POLYS,
             "# curve   k   multi-open proof              Ipa::create_proof (zk) alone   the front adds"]
    pre = b"bench_ipa_multiopen"
    for curve in a.curves.split(","):
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        for k in [int(x) for x in a.ks.split(",")]:
            n = 1 << k
            rnd = random.Random("bench-multiopen-%s-%d" % (curve, k))
            if curve == "bn254":
                d = torch.empty(64 * (n + 2), dtype=torch.uint8, device="cuda")
                ctx.sample_points_dev(k, n + 2, d.data_ptr())
                ctx.sync()
                gb = d.cpu().numpy().tobytes()
                dk = sv.IpaDecidingKey(ctx, gb[:64 * n])
            else:
                gb = pallas_points(ctx, rnd, n + 2)
                dk = ctx.ipa_dk_create(gb[:64 * n])
            hb, sb = gb[64 * n:64 * (n + 1)], gb[64 * (n + 1):]
            d_polys = device_scalars(torch, N_POLYS * n, 1000 + k)
            d_bar = device_scalars(torch, n, 2000 + k)
            one = lambda: int.from_bytes(scalars(rnd, 1), "little")  # noqa: E731
            x, w, w_last = one(), one(), one()
            blinds, f_blind, omega, omega_bar = [one() for _ in range(N_POLYS)], one(), one(), one()
            # the queries, their evaluations by the device
            pairs = [(p, 1) for p in range(N_POLYS)] + [(14, w), (15, w), (14, w_last)]
            r = field[curve]
            pts = torch.frombuffer(bytearray(b"".join((x * s % r).to_bytes(32, "little") for _, s in pairs)), dtype=torch.uint8).cuda()
            evs = torch.empty(32 * len(pairs), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for i, (p, _) in enumerate(pairs):
                P.eval_dev(ctx, d_polys.data_ptr() + 32 * n * p, n, pts.data_ptr() + 32 * i, evs.data_ptr() + 32 * i)
            ctx.sync()
            raw = evs.cpu().numpy().tobytes()
            queries = [(p, s, raw[32 * i:32 * i + 32]) for i, (p, s) in enumerate(pairs)]
            multi = lambda: MO.create_proof_dev(ctx, dk, hb, sb, d_polys.data_ptr(), N_POLYS, blinds, x, queries, f_blind,  # noqa: E731
                                                d_bar.data_ptr(), omega_bar, absorbed=pre)
            alone = lambda: CR.create_proof_dev(ctx, dk, hb, sb, d_polys.data_ptr(), n, x, omega, d_bar.data_ptr(), omega_bar,  # noqa: E731
                                                absorbed=pre)
            proof, _ = multi()
            assert len(proof) == MO.proof_bytes(k, 3)
            t_multi, t_alone = [], []
            for i in range(WARMUPS + RUNS):
                for fn, ts in ((multi, t_multi), (alone, t_alone)):
                    t0 = time.perf_counter()
                    fn()
                    if i >= WARMUPS:
                        ts.append((time.perf_counter() - t0) * 1e3)
            mm, ma = statistics.median(t_multi), statistics.median(t_alone)
            lines.append("%-7s %3d   %8.3f [%8.3f .. %8.3f]   %8.3f [%8.3f .. %8.3f]   %8.3f ms (x %.2f)"
                         % (curve, k, mm, min(t_multi), max(t_multi), ma, min(t_alone), max(t_alone), mm - ma, mm / ma))
            print(lines[-1], flush=True)
            dk.close()
            del d_polys, d_bar
        ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
