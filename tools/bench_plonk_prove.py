"""Times a whole PLONK prover session (snark_verifier_amd.host_plonk_prove) for circuit B of tests/plonk_prover_util.py at
k = 10, 16 and 20, next to its floor: the same number of bare commitments in one snarkv_g1_msm_pippenger_many_dev call.

The witness is made on the device beforehand and is not timed: random advice with c solved from the gate, sigma = identity
but for one copy (b[1] = b[2]: without any the permutation terms vanish identically and the third chunk of h is the zero
polynomial, whose commitment no transcript takes), fixed columns zero on the six unusable rows.  The SRS is n sampled points:
the proof is not verifiable, and the prover's own checks (the quotient's tail, the identity at z, the remainders of the
opening) do not involve it.  One untimed session gives the challenges the Z columns are made from; the transcript is a
function of the inputs, so every timed session squeezes the same ones.

A session is begin + the three phases + finish + destroy on the host clock, its device memory included.  Session and floor
alternate in one process: 3 warm-ups, then the median of 11 with [min .. max].

    python tools/bench_plonk_prove.py [--ks 10,16,20] [--out profiles/plonk_prove_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUPS, RUNS = 3, 11
COLS = 18
LAST = -6


def main():
    import torch

    import plonk_prover_util as PU
    import plonk_synth as S
    import snark_verifier_amd as sv
    from snark_verifier_amd import host_api as H
    from snark_verifier_amd import host_plonk_prove as HP
    from snark_verifier_amd import ntt, poly, poly_prod

    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    R = PU.R
    ctx = sv.Context(0)
    lines = ["# ms on the host clock: median of %d after %d warm-ups [min .. max]; session and floor alternate in one process" % (RUNS, WARMUPS),
             "# session: begin + 3 phases + finish + destroy, circuit B (17 columns, e = 2), witness columns prepared beforehand",
             "# floor: the same number of commitments (6 witness + 3 chunks + the opening's) as one g1_msm_pippenger_many_dev + sync",
             "#  k  scheme  msms   session                              floor                                /floor   device MiB"]

    def fe(v):
        return int(v % R).to_bytes(32, "little")

    def dev(raw):
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    for k in [int(x) for x in args.ks.split(",")]:
        n = 1 << k
        u = n + LAST
        col = 32 * n
        # values: 0 a, 1 b, 2 c | 3 q_a, 4 q_b, 5 q_c, 6 q_ab, 7 q_k, 8..10 sigma | 11 I | 12..14 products | 15..17 identities
        V = torch.zeros(col * COLS, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        at = lambda i: V.data_ptr() + col * i  # noqa: E731
        for seed, i in enumerate((0, 1, 3, 4, 6)):
            ctx.sample_scalars_dev(1000 + seed, n, at(i))
        ctx.sync()
        for i in (3, 4, 6):
            V[col * i + 32 * u:col * (i + 1)] = 0
        V[col * 5:col * 5 + 32 * u] = dev(fe(R - 1) * u)
        inst = [[11, 22]]
        V[col * 11:col * 11 + 64] = dev(fe(11) + fe(22))
        for j in range(3):  # delta^j w^i: the values of the polynomial delta^j X
            V[col * (15 + j) + 32:col * (15 + j) + 64] = dev(fe(pow(PU.CircuitB.DELTA, j, R)))
        torch.cuda.synchronize()
        ntt.ntt_dev(ctx, at(15), at(15), k, 3)
        ctx.sync()
        V[col * 8:col * 11] = V[col * 15:col * 18]
        V[col + 64:col + 96] = V[col + 32:col + 64]  # b[2] = b[1], and sigma_2 swaps the two cells
        V[col * 9 + 32:col * 9 + 64] = V[col * 16 + 64:col * 16 + 96]
        V[col * 9 + 64:col * 9 + 96] = V[col * 16 + 32:col * 16 + 64]
        torch.cuda.synchronize()
        poly_prod.mul_dev(ctx, at(3), at(0), n, at(12))
        poly_prod.mul_dev(ctx, at(4), at(1), n, at(13))
        poly_prod.mul_dev(ctx, at(0), at(1), n, at(14))
        poly_prod.mul_dev(ctx, at(6), at(14), n, at(14))
        poly.lincomb_dev(ctx, V, n, COLS, [12, 13, 14, 11], [1, 1, 1, 1], at(2))  # the gate solved for c (q_c = -1)
        d_pre = torch.zeros(col * 8, dtype=torch.uint8, device="cuda")
        d_srs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        d_w2 = torch.zeros(col * 3, dtype=torch.uint8, device="cuda")
        d_work = torch.zeros(col * 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.sync()
        d_pre.copy_(V[col * 3:col * 11])
        torch.cuda.synchronize()
        ntt.intt_dev(ctx, d_pre, d_pre, k, 8)
        ctx.sample_points_dev(7, n, d_srs.data_ptr())
        ctx.sample_scalars_dev(2000, n, d_w2.data_ptr() + 2 * col)
        ctx.sync()
        pr = PU.CircuitB(4).protocol  # the constraints; the domain and the commitments are this size's
        pr = dict(pr, domain=PU.P.Domain(k), preprocessed=[PU.O.G1_GEN] * 8)
        protocol = H.Protocol(S.pack_protocol(pr))
        plan = HP.plan(protocol)

        def session(mos, make_z):
            with HP.PlonkProver(protocol, ctx, d_srs, d_pre, inst, mos, HP.TRANSCRIPT_EVM) as p:
                ch = p.phase(V[:col * 3], HP.FORM_VALUES)
                ch += p.phase(None)
                if make_z:
                    poly_prod.perm_product_dev(ctx, V, n, COLS, [0, 1], [15, 16], [8, 9], ch[1], ch[2], d_work, d_w2.data_ptr())
                    poly_prod.perm_product_dev(ctx, V, n, COLS, [2], [17], [10], ch[1], ch[2], d_work, d_w2.data_ptr() + col,
                                               d_start=d_w2.data_ptr() + 32 * u)
                    ctx.sync()
                p.phase(d_w2, HP.FORM_VALUES)
                proof = p.finish()
            assert proof, "the bench witness does not satisfy circuit B"
            return proof

        for mos, name in ((HP.MOS_GWC19, "gwc19"), (HP.MOS_BDFG21, "bdfg21")):
            proof = session(mos, True)
            n_msm = 6 + 3 + (len({r for _, r in pr["queries"]}) if mos == HP.MOS_GWC19 else 2)
            d_out = torch.zeros(64 * n_msm, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            scal = [V.data_ptr() + col * (i % 7) for i in range(n_msm)]

            def floor():
                ctx.msm_pippenger_many_dev(scal, [d_srs.data_ptr()] * n_msm, [n] * n_msm, d_out.data_ptr())
                ctx.sync()

            ts, tf = [], []
            for it in range(WARMUPS + RUNS):
                t0 = time.perf_counter()
                again = session(mos, False)
                t1 = time.perf_counter()
                floor()
                t2 = time.perf_counter()
                assert again == proof
                if it >= WARMUPS:
                    ts.append(1e3 * (t1 - t0))
                    tf.append(1e3 * (t2 - t1))
            ms, mf = statistics.median(ts), statistics.median(tf)
            lines.append("  %2d  %-6s  %4d  %9.3f [%9.3f .. %9.3f]  %9.3f [%9.3f .. %9.3f]  %7.2f  %10.1f"
                         % (k, name, n_msm, ms, min(ts), max(ts), mf, min(tf), max(tf), ms / mf, plan["bytes"] / 2 ** 20))
            print(lines[-1], flush=True)
        del V, d_pre, d_srs, d_w2, d_work
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
