"""Times `Ipa::create_proof` (non-zk) through its two routes, alternating in one process:
    one-call   snark_verifier_amd.ipa_create.create_proof: Blake2b transcript on the device, one synchronisation
    session    the session of include/snarkv_ipa_prover.h driven from Python with a hashlib Blake2b transcript
on BN254 and pallas at k = 10, 16, 20: 3 warm-ups, then the median of 11 with [min .. max], ms per proof.

    python tools/bench_ipa_create.py [--ks 10,16,20] [--curves bn254,pallas] [--out FILE]

The record says per (curve, k) whether the one-call route is slower than the session beyond the observed spread (its fastest
run slower than the session's slowest).  Nothing routes on these numbers.

The kernel's own time comes from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_ipa_create.py --one-call-only --ks 10
    python tools/bench_ipa_create.py --kernel-trace DIR [--out FILE]
which prints the duration of every new kernel per launch (median [min .. max]) and, appended to --out, the same lines."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WARMUPS, RUNS = 3, 11
NEW_KERNELS = ["k_ipa_transcript_round", "k_ipa_transcript_open", "k_ipa_transcript_finish", "k_ipa_transcript_zk",
               "k_ipa_eval_partials", "k_ipa_eval_sub", "k_ipa_axpy", "k_ipa_fold_offsets"]


def kernel_trace(root, out):
    import csv

    by_name = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(d, f)) as fh:
                    for r in csv.DictReader(fh):
                        for k in NEW_KERNELS + ["k_ipa_xi_inv"]:
                            if k in r["Kernel_Name"]:
                                by_name.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["# kernels alone (rocprofv3 --kernel-trace): us per launch, median [min .. max] over the launches"]
    for k in sorted(by_name):
        t = by_name[k]
        lines.append("%-26s %4d launches  %8.1f [%8.1f .. %8.1f]" % (k, len(t), statistics.median(t), min(t), max(t)))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def scalars(rnd, n):
    """n canonical scalars for either field: 252 random bits each"""
    raw = bytearray(rnd.randbytes(32 * n))
    raw[31::32] = bytes(b & 0x0F for b in raw[31::32])
    return bytes(raw)


def pallas_points(ctx, rnd, count):
    """`count` points as two-term combinations of 64 sampled ones, 2^14 per segmented launch (no sampling loop in Python)"""
    import pallas as PA

    base = [PA.g1_to_bytes(p) for p in PA.sample_points(20, 64)]
    out = []
    for lo in range(0, count, 1 << 14):
        m = min(1 << 14, count - lo)
        pts = b"".join(base[rnd.randrange(64)] + base[rnd.randrange(64)] for _ in range(m))
        out.append(ctx.msm_batched(scalars(rnd, 2 * m), pts, list(range(0, 2 * m + 1, 2))))
    return b"".join(out)


def session_proof(P, T, cv, ctx, dk, pb, z, h, pre):
    t = T.Blake2bTranscript(cv)
    t.state.update(pre)
    xi0 = t.squeeze_challenge()
    xi = []
    with P.IpaProver(ctx, dk, pb, z, h, xi0) as s:
        for _ in range(dk.k):
            l, r = s.round()
            t.write_ec_point(P._from_pt(l))
            t.write_ec_point(P._from_pt(r))
            x = t.squeeze_challenge()
            s.fold(x)
            xi.append(x)
        u, c = s.finish()
    u = P._from_pt(u)
    t.write_ec_point(u)
    t.write_scalar(int.from_bytes(c, "little"))
    return t.finalize(), (xi, u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--one-call-only", action="store_true", help="a few proofs through the one-call route (for a kernel trace)")
    ap.add_argument("--kernel-trace", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_trace(a.kernel_trace, a.out)
    import torch

    import snark_verifier_amd as sv
    import transcript as T
    from snark_verifier_amd import ipa_create as CR
    from snark_verifier_amd import ipa_prover as P
    from snark_verifier_amd import pallas as PL

    lines = ["# Ipa::create_proof, non-zk, ms per proof: median of %d after %d warm-ups [min .. max]; the two routes alternate"
             % (RUNS, WARMUPS), "# curve   k   one-call                      session (hashlib transcript)   one-call / session"]
    pre = b"bench_ipa_create"
    for curve in a.curves.split(","):
        if curve == "bn254":
            import bn254 as cv

            ctx = sv.Context(0)
        else:
            import pallas as cv

            ctx = PL.PallasContext(0)
        for k in [int(x) for x in a.ks.split(",")]:
            n = 1 << k
            rnd = random.Random("bench-create-%s-%d" % (curve, k))
            if curve == "bn254":
                d = torch.empty(64 * (n + 1), dtype=torch.uint8, device="cuda")
                ctx.sample_points_dev(k, n + 1, d.data_ptr())
                ctx.sync()
                gb = d.cpu().numpy().tobytes()
                dk = sv.IpaDecidingKey(ctx, gb[:64 * n])
            else:
                gb = pallas_points(ctx, rnd, n + 1)
                dk = ctx.ipa_dk_create(gb[:64 * n])
            hb = gb[64 * n:]
            h = P._from_pt(hb)
            pb, z = scalars(rnd, n), int.from_bytes(scalars(rnd, 1), "little")
            one = lambda: CR.create_proof(ctx, dk, hb, None, pb, z, absorbed=pre)  # noqa: E731
            ses = lambda: session_proof(P, T, cv, ctx, dk, pb, z, h, pre)  # noqa: E731
            if a.one_call_only:
                for _ in range(WARMUPS + 3):
                    one()
                dk.close()
                continue
            assert one() == ses(), "the two routes disagree"
            t_one, t_ses = [], []
            for i in range(WARMUPS + RUNS):
                for fn, ts in ((one, t_one), (ses, t_ses)):
                    t0 = time.perf_counter()
                    fn()
                    if i >= WARMUPS:
                        ts.append((time.perf_counter() - t0) * 1e3)
            mo, ms = statistics.median(t_one), statistics.median(t_ses)
            verdict = "SLOWER beyond the spread" if min(t_one) > max(t_ses) else (
                "faster beyond the spread" if max(t_one) < min(t_ses) else "within the spread")
            lines.append("%-7s %3d   %8.3f [%8.3f .. %8.3f]   %8.3f [%8.3f .. %8.3f]   %5.2f  %s"
                         % (curve, k, mo, min(t_one), max(t_one), ms, min(t_ses), max(t_ses), mo / ms, verdict))
            print(lines[-1], flush=True)
            dk.close()
        ctx.close()
    if not a.one_call_only:
        text = "\n".join(lines)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
