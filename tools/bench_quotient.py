"""Times the quotient calls (snark_verifier_amd.quotient, columns resident on the device) on BN254 and pallas at extended
sizes k + e = 10, 16, 20, 24 with e = 2: `extend_dev` on the 11 columns of the small circuit of tests/quotient_util.py,
`eval_dev` on that circuit's program (29 instructions), on its gate alone (6) and on a 64-instruction program over two
columns, `div_vanishing_dev`, and `quotient_dev` on the circuit -- next to three yardsticks taken in the same process:

  (a) a device-to-device copy of one extended column (2^(k+e) x 32 bytes) times the columns the call reads and writes:
      extend 22 (11 padded, 11 transformed), eval the columns its program names + 1, div_vanishing 2, quotient_dev the sum of
      its steps + 2 for the inverse transform;
  (b) one forward transform of size k + e (`ntt.ntt_dev`);
  (c) for the gate row: the same expression q_mul (a b - c) + q_add (a + b - c) built from the existing `poly_mul_dev` and
      `poly_lincomb_dev` on the extended columns, six calls with three intermediate columns.

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise).

    python tools/bench_quotient.py [--logs 10,16,20,24] [--curves bn254,pallas] [--out FILE]

`/copy` is the call's time over the copies, `/ntt` over the transform, `/calls` over (c).  The values are random, not a
satisfied witness: the kernels do the same work on either.  Nothing routes on these numbers and none is a pass mark."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_ipa_multiopen import device_scalars  # noqa: E402

WARMUPS, RUNS = 3, 11
E = 2


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
    ap.add_argument("--logs", default="10,16,20,24")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import quotient_util as QU
    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt as N
    from snark_verifier_amd import pallas as PL
    from snark_verifier_amd import poly as PO
    from snark_verifier_amd import poly_prod as P
    from snark_verifier_amd import quotient as Q

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max]" % (RUNS, WARMUPS),
             "# log = k + e, e = %d; copy: device-to-device copy of one extended column x the columns the call reads and writes;" % E,
             "# ntt: one forward transform of 2^log; calls: the gate from poly_mul_dev / poly_lincomb_dev, six calls",
             "# curve  log  call          instr  cols   call                               copy x cols                        "
             "ntt                                  /copy    /ntt  /calls"]
    for curve in a.curves.split(","):
        r = QU.FIELD[curve]
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        s = QU.zeta(curve)
        s_inv = pow(s, -1, r)
        c = QU.Circuit(curve, 4)  # its programs and challenges; the columns below are random
        circuit, gate = c.program(Q), c.program(Q, permutation=False)
        long = (QU.pack_program(Q, QU.random_program(Q, random.Random("bench-quotient"), 64, 2, 4)), [3, 5, 7, r - 1])
        for log in [int(x) for x in a.logs.split(",")]:
            k, n, n_ext = log - E, 1 << (log - E), 1 << log
            cols = QU.COLS
            d_coeffs = device_scalars(torch, cols * n, 5000 + log)
            d_ext = torch.empty(32 * (cols + 3) * n_ext, dtype=torch.uint8, device="cuda")  # the columns and three temporaries
            d_work = torch.empty(32 * cols * n_ext, dtype=torch.uint8, device="cuda")
            d_out = torch.empty(32 * n_ext, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            Q.extend_dev(ctx, d_coeffs, k, E, cols, s, d_ext)
            ctx.sync()
            col = lambda j: d_ext.data_ptr() + 32 * n_ext * j  # noqa: E731
            d_col = d_ext[:32 * n_ext]
            t_once = timed(lambda: d_out.copy_(d_col), torch.cuda.synchronize)
            t_ntt = timed(lambda: N.ntt_dev(ctx, d_col, d_out, log), ctx.sync)
            t0, t1, t2 = cols, cols + 1, cols + 2

            def by_calls():
                P.mul_dev(ctx, col(QU.COL_A), col(QU.COL_B), n_ext, col(t0))
                PO.lincomb_dev(ctx, d_ext, n_ext, cols + 3, [t0, QU.COL_C], [1, r - 1], col(t1))
                P.mul_dev(ctx, col(t1), col(QU.COL_QM), n_ext, col(t1))
                PO.lincomb_dev(ctx, d_ext, n_ext, cols + 3, [QU.COL_A, QU.COL_B, QU.COL_C], [1, 1, r - 1], col(t0))
                P.mul_dev(ctx, col(t0), col(QU.COL_QA), n_ext, col(t0))
                PO.lincomb_dev(ctx, d_ext, n_ext, cols + 3, [t0, t1], [1, 1], col(t2))

            t_calls = timed(by_calls, ctx.sync)
            Q.eval_dev(ctx, d_ext, k, E, cols, gate, d_out)
            ctx.sync()
            assert bytes(d_out.cpu().numpy()) == bytes(d_ext[32 * n_ext * t2:32 * n_ext * (t2 + 1)].cpu().numpy()), "the gate, both ways"
            calls = (
                ("extend", 0, 2 * cols, lambda: Q.extend_dev(ctx, d_coeffs, k, E, cols, s, d_work)),
                ("eval gate", len(gate), 5 + 1, lambda: Q.eval_dev(ctx, d_ext, k, E, cols, gate, d_out)),
                ("eval circuit", len(circuit), cols + 1, lambda: Q.eval_dev(ctx, d_ext, k, E, cols, circuit, d_out)),
                ("eval 64", 64, 2 + 1, lambda: Q.eval_dev(ctx, d_ext, k, E, 2, long, d_out)),
                ("div_vanishing", 0, 2, lambda: Q.div_vanishing_dev(ctx, d_out, k, E, s, d_out)),
                ("quotient", len(circuit), 2 * cols + cols + 1 + 2 + 2,
                 lambda: Q.quotient_dev(ctx, d_coeffs, k, E, cols, circuit, s, s_inv, d_work, d_out)),
            )
            for name, instr, width, fn in calls:
                t = timed(fn, ctx.sync)
                t_copy = tuple(width * x for x in t_once)
                lines.append("%-7s %3d  %-13s %5d %5d   %s   %s   %s   %7.2f %7.2f %7s" % (
                    curve, log, name, instr, width, fmt(t), fmt(t_copy), fmt(t_ntt), t[0] / t_copy[0], t[0] / t_ntt[0],
                    "%7.2f" % (t[0] / t_calls[0]) if name == "eval gate" else "-"))
                print(lines[-1], flush=True)
                if name == "eval gate":
                    lines.append("%-7s %3d  %-13s %5d %5d   %s" % (curve, log, "gate by calls", 6, 6 * 3, fmt(t_calls)))
                    print(lines[-1], flush=True)
            del d_coeffs, d_ext, d_work, d_out, d_col
        ctx.close()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
