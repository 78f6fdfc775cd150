"""Times the two KZG multi-open provers (snark_verifier_amd.kzg_multiopen, polynomials and base resident on the device) and the
batched evaluation (snark_verifier_amd.poly_batch) on BN254 at k = 10, 16, 20, each next to its floor, the pairs alternating
in one process: 3 warm-ups, then the median of 11 with [min .. max], ms per call on the host clock around work that ends in a
synchronise.

    python tools/bench_kzg_multiopen.py [--ks 10,16,20] [--out FILE]

The query shape is oracle/kzg.py::standard_plonk_queries: 17 polynomials, all opened at z, three also at a second rotation
and two at a third -- 22 queries, 3 Gwc19 sets, 4 Bdfg21 sets of 1, 2, 3 and 2 points.  The pairs:

    gwc19       gwc19_create_proof_dev                   | 3 bare commitments in one msm_pippenger_many_dev, one synchronise
    bdfg21      bdfg21_create_proof_dev                  | 2 bare commitments by msm_pippenger_dev, a synchronise after each
    eval_many   the 22 evaluations in one eval_many_dev  | the loop of 22 poly.eval_dev calls, one synchronise

A floor is the commitments alone on the same polynomials over the same base: what the scheme adds is its linear
combinations, divisions and host work.  The base is sampled points, not the powers of a secret: the time of an MSM does not
depend on it, and the outputs are not verified here (tests/test_gpu_kzg_multiopen.py does that).  Nothing routes on these
numbers, and none is a pass mark."""
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

from bench_ipa_multiopen import device_scalars  # noqa: E402

WARMUPS, RUNS = 3, 11
N_POLYS = 17


def timed_pairs(pairs):
    """[(name, fn_a, fn_b)] -> {name: (times a, times b)}: every pair alternates, the pairs one after the other"""
    out = {}
    for name, fa, fb in pairs:
        ta, tb = [], []
        for i in range(WARMUPS + RUNS):
            for fn, ts in ((fa, ta), (fb, tb)):
                t0 = time.perf_counter()
                fn()
                if i >= WARMUPS:
                    ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = (ta, tb)
    return out


def fmt(ts):
    return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import kzg_multiopen as KM
    from snark_verifier_amd import poly as P
    from snark_verifier_amd import poly_batch as PB

    import bn254 as BN
    import kzg as K

    r = BN.R
    lines = ["# ms per call on the host clock: median of %d after %d warm-ups [min .. max]; the two calls of a pair alternate" % (RUNS, WARMUPS),
             "# BN254, %d polynomials on the device, 22 queries: 3 Gwc19 sets, 4 Bdfg21 sets (1 | 2 | 3 | 2 points)" % N_POLYS,
             "#   k  pair        the call                         its floor                        call - floor   ranges"]
    ctx = sv.Context(0)
    for k in [int(x) for x in a.ks.split(",")]:
        n = 1 << k
        rnd = random.Random("bench-kzg-multiopen-%d" % k)
        d_srs = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        ctx.sample_points_dev(k, n, d_srs.data_ptr())
        d_polys = device_scalars(torch, N_POLYS * n, 3000 + k)
        z, v, mu, gamma, z_prime = (rnd.randrange(1, r) for _ in range(5))
        pairs = K.standard_plonk_queries(rnd, N_POLYS)
        shifts = sorted({sh for _, sh in pairs})
        d_points = torch.frombuffer(bytearray(b"".join((z * sh % r).to_bytes(32, "little") for sh in shifts)), dtype=torch.uint8).cuda()
        q_poly, q_point = [p for p, _ in pairs], [shifts.index(sh) for _, sh in pairs]
        d_evs = torch.empty(32 * len(pairs), dtype=torch.uint8, device="cuda")
        d_evs1 = torch.empty(32 * len(pairs), dtype=torch.uint8, device="cuda")
        d_out = torch.empty(64 * 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.sync()
        polys_at = [d_polys.data_ptr() + 32 * n * p for p in range(N_POLYS)]

        def eval_many():
            PB.eval_many_dev(ctx, d_polys, n, N_POLYS, d_points, len(shifts), q_poly, q_point, d_evs)
            ctx.sync()

        def eval_loop():
            for i, (p, t) in enumerate(zip(q_poly, q_point)):
                P.eval_dev(ctx, polys_at[p], n, d_points.data_ptr() + 32 * t, d_evs1.data_ptr() + 32 * i)
            ctx.sync()

        eval_many()
        eval_loop()
        raw = d_evs.cpu().numpy().tobytes()
        assert raw == d_evs1.cpu().numpy().tobytes()
        queries = [(p, sh, raw[32 * i:32 * i + 32]) for i, (p, sh) in enumerate(pairs)]
        assert KM.n_sets(KM.MOS_GWC19, queries) == 3 and KM.n_sets(KM.MOS_BDFG21, queries) == 4

        def gwc19():
            assert len(KM.gwc19_create_proof_dev(ctx, d_srs, d_polys, n, N_POLYS, z, queries, v)) == 3

        def gwc19_floor():
            ctx.msm_pippenger_many_dev(polys_at[:3], [d_srs.data_ptr()] * 3, [n] * 3, d_out.data_ptr())
            ctx.sync()

        def bdfg21():
            KM.bdfg21_create_proof_dev(ctx, d_srs, d_polys, n, N_POLYS, z, queries, mu, gamma, lambda w: z_prime)

        def bdfg21_floor():
            for i in range(2):
                ctx.msm_pippenger_dev(polys_at[i], d_srs.data_ptr(), n, d_out.data_ptr() + 64 * i)
                ctx.sync()

        res = timed_pairs([("gwc19", gwc19, gwc19_floor), ("bdfg21", bdfg21, bdfg21_floor), ("eval_many", eval_many, eval_loop)])
        for name, (ta, tb) in res.items():
            apart = max(ta) < min(tb) or max(tb) < min(ta)
            lines.append("%5d  %-10s  %s   %s   %+9.3f ms   %s" % (k, name, fmt(ta), fmt(tb), statistics.median(ta) - statistics.median(tb),
                                                                  "apart" if apart else "OVERLAP"))
            print(lines[-1], flush=True)
        del d_srs, d_polys
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
