"""Times a whole PLONK prover session on pallas (snark_verifier_amd.host_plonk_prove_pallas) for circuit B of
tests/plonk_prover_pallas_util.py at k = 10 and 16, next to its floor: the commitments and the opening called directly -- one
snarkv_pallas_ipa_commit_blinded_batch_dev with as many commitments as the session makes (6 witness + 3 chunks), plus one
snarkv_pallas_ipa_multiopen_create_proof_dev over the same sixteen polynomials and the protocol's queries.

The method is tools/bench_plonk_prove.py's.  The witness is made on the device beforehand and is not timed: random advice with
c solved from the gate, sigma = identity but for one copy (b[1] = b[2]), fixed columns zero on the six unusable rows.  The key
is the n points G, 2 G, .. n G: the proofs are not verified here, and the prover's own checks (the quotient's tail, the
identity at z, the remainders of the opening) do not involve the key.  One untimed session gives the challenges the Z columns
are made from; the transcript is a function of the inputs, so every timed session squeezes the same ones.  Blinds are fixed
non-zero scalars.

A session is begin + the three phases + finish + destroy on the host clock, its device memory included.  Session and floor
alternate in one process: 3 warm-ups, then the median of 11 with [min .. max].  The BN254 session's recorded numbers
(profiles/plonk_prove_bench.txt) are printed beside the table for orientation only: another curve, another scheme.

    python tools/bench_plonk_prove_pallas.py [--ks 10,16] [--out profiles/plonk_prove_pallas_bench.txt]"""
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


def key_points(PA, n):
    """G, 2 G, .. n G as bytes: affine additions with one shared inversion per level of doubling"""
    pts = [PA.G1_GEN]
    while len(pts) < n:  # pts + [len(pts)] G, all the x differences inverted together
        step = pts[-1]  # = len(pts) G; the last sum is its doubling, done apart
        dx = [(step[0] - p[0]) % PA.P for p in pts[:-1]] + [1]
        pre, acc = [], 1
        for d in dx:
            pre.append(acc)
            acc = acc * d % PA.P
        inv, out = pow(acc, -1, PA.P), [None] * len(pts)
        for i in range(len(pts) - 1, -1, -1):
            di = inv * pre[i] % PA.P
            inv = inv * dx[i] % PA.P
            lam = (step[1] - pts[i][1]) * di % PA.P
            x = (lam * lam - pts[i][0] - step[0]) % PA.P
            out[i] = (x, (lam * (pts[i][0] - x) - pts[i][1]) % PA.P)
        out[-1] = PA.g1_double(step)
        pts += out
    return b"".join(PA.g1_to_bytes(p) for p in pts[:n])


def main():
    import torch

    import pallas as PA
    import plonk_prover_pallas_util as PP
    import plonk_synth as S
    from snark_verifier_amd import host_api_pallas as HA
    from snark_verifier_amd import g1_ntt
    from snark_verifier_amd import host_plonk_prove_pallas as HP
    from snark_verifier_amd import host_plonk_prove_pallas_ci as HC
    from snark_verifier_amd import ipa_commit_blinded, ipa_multiopen, ntt, poly, poly_batch, poly_prod
    from snark_verifier_amd import pallas as PL

    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    R = PA.R
    ctx = PL.PallasContext(0)
    lines = ["# ms on the host clock: median of %d after %d warm-ups [min .. max]; session and floor alternate in one process" % (RUNS, WARMUPS),
             "# session: begin + 3 phases + finish + destroy, circuit B on pallas (17 columns, e = 2), witness columns prepared beforehand",
             "# floor: ipa_commit_blinded_batch_dev of 9 polynomials + sync, then ipa_multiopen_create_proof_dev over the 16 polynomials",
             "#        and the protocol's 20 queries, both called directly",
             "#  k  commits  sets   session                              floor                                /floor   device MiB"]

    def fe(v):
        return int(v % R).to_bytes(32, "little")

    def dev(raw):
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    def random_scalars(seed, n):
        """n scalars below 2^254 < r, as bytes on the device"""
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        t = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        t[:, 31] &= 0x3F
        return t.reshape(-1)

    h_pt, s_pt = PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, 0xA11CE)), PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, 0xB0B))
    for k in [int(x) for x in args.ks.split(",")]:
        n = 1 << k
        u = n + LAST
        col = 32 * n
        # values: 0 a, 1 b, 2 c | 3 q_a, 4 q_b, 5 q_c, 6 q_ab, 7 q_k, 8..10 sigma | 11 I | 12..14 products | 15..17 identities
        V = torch.zeros(col * COLS, dtype=torch.uint8, device="cuda")
        for seed, i in enumerate((0, 1, 3, 4, 6)):
            V[col * i:col * (i + 1)] = random_scalars(1000 + seed, n)
        at = lambda i: V.data_ptr() + col * i  # noqa: E731
        for i in (3, 4, 6):
            V[col * i + 32 * u:col * (i + 1)] = 0
        V[col * 5:col * 5 + 32 * u] = dev(fe(R - 1) * u)
        inst = [[11, 22]]
        V[col * 11:col * 11 + 64] = dev(fe(11) + fe(22))
        for j in range(3):  # delta^j w^i: the values of the polynomial delta^j X
            V[col * (15 + j) + 32:col * (15 + j) + 64] = dev(fe(pow(PP.CircuitB.DELTA, j, R)))
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
        d_w2 = torch.zeros(col * 3, dtype=torch.uint8, device="cuda")
        d_work = torch.zeros(col * 2, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.sync()
        d_pre.copy_(V[col * 3:col * 11])
        d_w2[2 * col:] = random_scalars(2000, n)
        d_pbar = random_scalars(3000, n)
        torch.cuda.synchronize()
        ntt.intt_dev(ctx, d_pre, d_pre, k, 8)
        ctx.sync()
        g_raw = key_points(PA, n)
        dk = ctx.ipa_dk_create(g_raw)
        with PP.on_pallas():
            pr = PP.CircuitB(4).protocol  # the constraints; the domain and the commitments are this size's
            pr = dict(pr, domain=PP.P.Domain(k), preprocessed=[PA.G1_GEN] * 8)
            protocol = HA.Protocol(S.pack_protocol(pr))
            shifts = [pr["domain"].rotate_scalar(1, rot) for _, rot in pr["queries"]]
            n_sets = len(PP.K.bdfg21_query_sets([(p, sh, 0) for (p, _), sh in zip(pr["queries"], shifts)]))
            # the same protocol as halo2 states it over IPA: the instance column committed over the first points of the key's
            # Lagrange basis (made on the device from the resident key), constant s, and its polynomial queried at z
            d_lag = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            g1_ntt.dk_lagrange_dev(ctx, dk, d_lag)
            ctx.sync()
            lag = d_lag[:128].cpu().numpy().tobytes()
            del d_lag
            ick = {"bases": [PA.g1_from_bytes(lag[:64]), PA.g1_from_bytes(lag[64:])], "constant": PA.g1_from_bytes(s_pt)}
            pr_ci = dict(pr, instance_committing_key=ick, evaluations=pr["evaluations"] + [(8, 0)], queries=pr["queries"] + [(8, 0)])
            protocol_ci = HA.Protocol(S.pack_protocol(pr_ci))
        plan = HP.plan(protocol)
        pre_blinds, w_blinds, z_blinds, chunk_blinds = [1] * 8, [101, 102, 103], [104, 105, 106], [107, 108, 109]
        f_blind, omega_bar = 110, 111

        def session(make_z, committed=False):
            # the challenges differ between the two transcripts, and with them the Z columns: each flavour has its own
            mod, prot, w2 = (HC, protocol_ci, d_w2_ci) if committed else (HP, protocol, d_w2)
            with mod.PlonkProver(prot, ctx, dk, h_pt, s_pt, d_pre, pre_blinds, inst) as p:
                ch = p.phase(V[:col * 3], w_blinds, HP.FORM_VALUES)
                ch += p.phase(None)
                if make_z:
                    poly_prod.perm_product_dev(ctx, V, n, COLS, [0, 1], [15, 16], [8, 9], ch[1], ch[2], d_work, w2.data_ptr())
                    poly_prod.perm_product_dev(ctx, V, n, COLS, [2], [17], [10], ch[1], ch[2], d_work, w2.data_ptr() + col,
                                               d_start=w2.data_ptr() + 32 * u)
                    ctx.sync()
                p.phase(w2, z_blinds, HP.FORM_VALUES)
                proof, _ = p.finish(chunk_blinds, f_blind, d_pbar, omega_bar)
            assert proof, "the bench witness does not satisfy circuit B"
            return proof

        proof = session(True)
        d_w2_ci = d_w2.clone()
        torch.cuda.synchronize()
        proof_ci = session(True, committed=True)
        # (no verifier here: the bench protocol's `preprocessed` are placeholders, as for the plain session; acceptance of
        # such proofs is tests/test_gpu_plonk_prove_pallas_ci.py's)
        assert proof_ci != proof and len(proof_ci) == len(proof) + 32
        # the floor's inputs: sixteen polynomials as coefficients (8 preprocessed, the instance's, 6 witness, and one more in the
        # quotient's place), the protocol's queries with their true evaluations at x * shift
        D = torch.zeros(col * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        D[:col * 8] = d_pre
        D[col * 8:col * 9] = V[col * 11:col * 12]
        D[col * 9:col * 12] = V[:col * 3]
        D[col * 12:col * 15] = d_w2
        D[col * 15:] = V[col * 12:col * 13]
        torch.cuda.synchronize()
        ntt.intt_dev(ctx, D.data_ptr() + col * 8, D.data_ptr() + col * 8, k, 7)
        x = 0x1234567 % R
        distinct = sorted(set(shifts))
        d_points = dev(b"".join(fe(x * sh) for sh in distinct))
        d_evals = torch.zeros(32 * len(shifts), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        poly_batch.eval_many_dev(ctx, D, n, 16, d_points, len(distinct), [p for p, _ in pr["queries"]], [distinct.index(sh) for sh in shifts], d_evals)
        ctx.sync()
        ev = d_evals.cpu().numpy().tobytes()
        queries = [(p, sh, ev[32 * i:32 * i + 32]) for i, ((p, _), sh) in enumerate(zip(pr["queries"], shifts))]
        blinds16 = pre_blinds + [0] + w_blinds + z_blinds + [112]
        d_cm = torch.zeros(64 * 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def floor():
            ipa_commit_blinded.commit_blinded_batch_dev(ctx, dk, s_pt, D.data_ptr() + col * 7, n, 9, w_blinds + z_blinds + chunk_blinds, d_cm)
            ctx.sync()
            return ipa_multiopen.create_proof_dev(ctx, dk, h_pt, s_pt, D.data_ptr(), 16, blinds16, x, queries, f_blind, d_pbar.data_ptr(), omega_bar)

        opened = floor()
        ts, tf, tc = [], [], []
        for it in range(WARMUPS + RUNS):
            t0 = time.perf_counter()
            again = session(False)
            t1 = time.perf_counter()
            again_opened = floor()
            t2 = time.perf_counter()
            again_ci = session(False, committed=True)
            t3 = time.perf_counter()
            assert again == proof and again_opened == opened and again_ci == proof_ci
            if it >= WARMUPS:
                ts.append(1e3 * (t1 - t0))
                tf.append(1e3 * (t2 - t1))
                tc.append(1e3 * (t3 - t2))
        ms, mf = statistics.median(ts), statistics.median(tf)
        lines.append("  %2d  %7d  %4d  %9.3f [%9.3f .. %9.3f]  %9.3f [%9.3f .. %9.3f]  %7.2f  %10.1f"
                     % (k, 9, n_sets, ms, min(ts), max(ts), mf, min(tf), max(tf), ms / mf, plan["bytes"] / 2 ** 20))
        print(lines[-1], flush=True)
        mc = statistics.median(tc)
        lines.append("# %2d  the session with committed instances (host_plonk_prove_pallas_ci: one more commitment and a synchronisation in"
                     " begin, 21 queries)  %9.3f [%9.3f .. %9.3f]  /session %5.2f" % (k, mc, min(tc), max(tc), mc / ms))
        print(lines[-1], flush=True)
        dk.close()
        del V, D, d_pre, d_w2, d_work, d_pbar
        torch.cuda.empty_cache()
    recorded = os.path.join(ROOT, "profiles", "plonk_prove_bench.txt")
    if os.path.exists(recorded):
        lines.append("# for orientation only -- the BN254 / KZG session as recorded in profiles/plonk_prove_bench.txt (its floor is a")
        lines.append("# batch of bare MSMs; another curve, another scheme: no ratio between the two tables means anything):")
        lines += ["#   " + ln.rstrip() for ln in open(recorded) if ln.split()[:1] and ln.split()[0] in ("10", "16")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
