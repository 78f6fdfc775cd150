"""Times the column products (snark_verifier_amd.poly_prod, columns resident on the device) on BN254 and pallas at
n = 1, 2^10, 2^16, 2^20, 2^24: the batch inversion, the grand product and the permutation product with three columns, next to
two yardsticks taken in the same process:

  (a) a device-to-device copy of the n * 32 bytes of one column, times the number of sweeps the call makes over data of that
      size: what moving the data once per sweep costs.  Sweeps: batch_invert 2 (totals up, inverses down), grand_product 2,
      perm_product 7 (two affine products, the inversion, the product, the grand product);
  (b) one forward transform of the same size (`ntt.ntt_dev`; n = 1 is the identity).

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise).

    python tools/bench_poly_prod.py [--ks 0,10,16,20,24] [--curves bn254,pallas] [--out FILE]

The n = 1 row is the latency floor of a call; for the inversion that is one Fermat chain on one lane.  `/copy` is the call's
time over the copies, `/ntt` over the transform.  Nothing routes on these numbers and none is a pass mark."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ipa_multiopen import device_scalars  # noqa: E402

WARMUPS, RUNS = 3, 11
SWEEPS = {"batch_invert": 2, "grand_product": 2, "perm_product": 7}
COLUMNS = 3


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
    ap.add_argument("--ks", default="0,10,16,20,24")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import ntt as N
    from snark_verifier_amd import pallas as PL
    from snark_verifier_amd import poly_prod as P

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max]" % (RUNS, WARMUPS),
             "# copy: device-to-device copy of one column (n x 32 bytes) x the sweeps of the call; ntt: one forward transform of n",
             "# perm_product: %d columns (v, id, sigma each), work and z apart from them" % COLUMNS,
             "# curve   k  call          sweeps   call                               copy x sweeps                      "
             "ntt                                  /copy    /ntt"]
    for curve in a.curves.split(","):
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        for k in [int(x) for x in a.ks.split(",")]:
            n = 1 << k
            d_polys = device_scalars(torch, 3 * COLUMNS * n, 4000 + k)
            d_work = torch.empty(2 * 32 * n, dtype=torch.uint8, device="cuda")
            d_out = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
            d_tot = torch.empty(32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            d_col = d_polys[:32 * n]
            iv, iid, isg = ([COLUMNS * j + i for i in range(COLUMNS)] for j in range(3))
            t_once = timed(lambda: d_out.copy_(d_col), torch.cuda.synchronize)
            t_ntt = timed(lambda: N.ntt_dev(ctx, d_col, d_out, k), ctx.sync)
            calls = (
                ("batch_invert", lambda: P.batch_invert_dev(ctx, d_col, n, d_out)),
                ("grand_product", lambda: P.grand_product_dev(ctx, d_col, n, d_out, d_total=d_tot)),
                ("perm_product", lambda: P.perm_product_dev(ctx, d_polys, n, 3 * COLUMNS, iv, iid, isg, 3, 5, d_work, d_out,
                                                            d_total=d_tot)),
            )
            for name, fn in calls:
                t = timed(fn, ctx.sync)
                t_copy = tuple(SWEEPS[name] * x for x in t_once)
                lines.append("%-7s %3d  %-13s %5d   %s   %s   %s   %7.2f %7.2f" % (
                    curve, k, name, SWEEPS[name], fmt(t), fmt(t_copy), fmt(t_ntt), t[0] / t_copy[0], t[0] / t_ntt[0]))
                print(lines[-1], flush=True)
            del d_polys, d_work, d_out
        ctx.close()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
