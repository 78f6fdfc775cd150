"""Times the IPA prover on the device (snark_verifier_amd.ipa_prover): ms per `Ipa::create_proof` (non-zk) at
k = 10, 16, 20 on BN254 and pallas, and its split -- the round calls (inner products + the two MSMs + the L / R
combination, synchronous), the folds (scalar fold + base fold, timed to a context sync), the host transcript
between the calls -- plus `snarkv_ipa_as_combine_dev` for m = 10.

    python tools/bench_ipa_prover.py [--ks 10,16,20] [--reps 3] [--naive-max N]

--naive-max sets SNARKV_IPA_NAIVE_MAX (the MSM size up to which a round uses the naive segmented kernels instead of
the Pippenger) for this process; run it twice to compare.  --rounds-only prints the per-half round time only.
One JSON line per measurement."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--naive-max", type=int, default=None)
    ap.add_argument("--rounds-only", action="store_true")
    ap.add_argument("--curves", default="bn254,pallas")
    a = ap.parse_args()
    if a.naive_max is not None:
        os.environ["SNARKV_IPA_NAIVE_MAX"] = str(a.naive_max)
    import torch

    import snark_verifier_amd as sv
    import transcript as T
    from snark_verifier_amd import ipa_prover as P
    from snark_verifier_amd import pallas as PL

    for curve in a.curves.split(","):
        if curve == "bn254":
            ctx, r = sv.Context(0), P.R_BN254
            mk_dk = lambda g: sv.IpaDecidingKey(ctx, g)  # noqa: E731
            mk_t = T.EvmTranscript
        else:
            import pallas as PA

            ctx, r = PL.PallasContext(0), P.R_PALLAS
            mk_dk = ctx.ipa_dk_create  # noqa: E731
            mk_t = lambda: T.Blake2bTranscript(PA)  # noqa: E731
        for k in [int(x) for x in a.ks.split(",")]:
            n = 1 << k
            if curve == "bn254":
                d = torch.empty(64 * (n + 1), dtype=torch.uint8, device="cuda")
                ctx.sample_points_dev(k, n + 1, d.data_ptr())
                ctx.sync()
                gb = d.cpu().numpy().tobytes()
            else:
                import pallas as PA

                # distinct points up to k = 16; at k = 20 (pure-Python sampling) 65 537 distinct points repeated: the
                # record labels those rows (`key`)
                m_pts = min(n + 1, (1 << 16) + 1)
                base = PA.sample_points(k, m_pts)
                gb = b"".join(PA.g1_to_bytes(base[i % m_pts]) for i in range(n + 1))
            h = (int.from_bytes(gb[64 * n:64 * n + 32], "little"), int.from_bytes(gb[64 * n + 32:], "little"))
            dk = mk_dk(gb[:64 * n])
            rnd = random.Random(k)
            p = [rnd.randrange(r) for _ in range(n)]
            pb = b"".join(x.to_bytes(32, "little") for x in p)
            z = rnd.randrange(r)
            best = None
            for _ in range(a.reps):
                t = mk_t()
                t_round = t_fold = t_host = 0.0
                per_half = []
                t0 = time.perf_counter()
                xi0 = t.squeeze_challenge()
                with P.IpaProver(ctx, dk, pb, z, h, xi0) as s:
                    t_begin = time.perf_counter() - t0
                    for i in range(k):
                        a0 = time.perf_counter()
                        l, rr = s.round()
                        a1 = time.perf_counter()
                        t.write_ec_point(P._from_pt(l))
                        t.write_ec_point(P._from_pt(rr))
                        x = t.squeeze_challenge()
                        a2 = time.perf_counter()
                        s.fold(x)
                        ctx.sync()
                        a3 = time.perf_counter()
                        t_round += a1 - a0
                        t_host += a2 - a1
                        t_fold += a3 - a2
                        per_half.append((n >> (i + 1), round((a1 - a0) * 1e3, 4)))
                    u, c = s.finish()
                total = time.perf_counter() - t0
                rec = dict(curve=curve, k=k, ms_total=round(total * 1e3, 3), ms_begin=round(t_begin * 1e3, 3),
                           ms_rounds=round(t_round * 1e3, 3), ms_folds=round(t_fold * 1e3, 3),
                           ms_transcript=round(t_host * 1e3, 3), naive_max=os.environ.get("SNARKV_IPA_NAIVE_MAX", "4096"),
                           key="distinct" if curve == "bn254" or k <= 16 else "65537 distinct points repeated")
                if a.rounds_only:
                    rec = dict(curve=curve, k=k, naive_max=rec["naive_max"], round_ms_by_half=per_half)
                if best is None or total < best[0]:
                    best = (total, rec)
            print(json.dumps(best[1]), flush=True)
            if not a.rounds_only and k >= 10:
                m = 10
                xis = [[rnd.randrange(r) for _ in range(k)] for _ in range(m)]
                d_h = torch.empty(32 << k, dtype=torch.uint8, device="cuda")
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    P.as_combine_dev(ctx, xis, 7, (3, 5), d_h.data_ptr())
                    ts.append(time.perf_counter() - t0)
                print(json.dumps(dict(curve=curve, k=k, as_combine_m=m, ms=round(min(ts) * 1e3, 3))), flush=True)
            dk.close()


if __name__ == "__main__":
    main()
