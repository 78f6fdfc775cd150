"""Times `quotient.cosets_dev` (the quotient one coset of the small domain at a time, include/snarkv_quotient_cosets.h) next to
`quotient.quotient_dev`, which is the yardstick, on BN254 and pallas: the 11 columns and the 29-instruction program of the
small circuit of tests/quotient_util.py at log = k + e = 16, 20, 24 with e = 2 and at log = 24 with e = 3.

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise); the two calls alternate in one
process, each on a context of its own.  After the timing the two outputs are compared byte for byte, and the row says so.

Memory per shape: `alloc` is what the caller allocates for the call (work + h; arithmetic), `ctx` is what the context grew by
on its first call of the shape -- the device's free memory before the call and after it, on a context that has run nothing
before: every (curve, shape, route) gets a fresh one.  Before a curve's first shape both calls run once at k = 1 on a
context that is then closed, so that what the runtime allocates once per process (the library's code, its own pools) is not
counted as the first row's scratch.

    python tools/bench_quotient_cosets.py [--shapes 16:2,20:2,24:2,24:3] [--curves bn254,pallas] [--out FILE]

The values are random, not a satisfied witness: the kernels do the same work on either.  Nothing routes on these numbers and
none is a pass mark."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_ipa_multiopen import device_scalars  # noqa: E402

WARMUPS, RUNS = 3, 11
MIB = 1 << 20


def fmt(ts):
    return "%9.3f [%9.3f .. %9.3f]" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:2,20:2,24:2,24:3")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import quotient_util as QU
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL
    from snark_verifier_amd import quotient as Q

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max], the two calls alternating" % (RUNS, WARMUPS),
             "# log = k + e; 11 columns, 29 instructions; MiB: alloc = work + h as the caller allocates them, ctx = what the context",
             "# grew by on its first call (free device memory before and after, a fresh context per route and shape)",
             "# curve  log  e   quotient_dev                       quotient_cosets_dev                cosets/dev   "
             "alloc dev  alloc cosets    ctx dev  ctx cosets   outputs"]
    for curve in a.curves.split(","):
        r = QU.FIELD[curve]
        s = QU.zeta(curve)
        s_inv = pow(s, -1, r)
        prog = QU.Circuit(curve, 4).program(Q)  # its program and challenges; the columns below are random
        cols = QU.COLS
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)  # the once-per-process allocations (see above)
        d_small = device_scalars(torch, cols * 2, 6999)
        d_tmp = torch.empty(32 * (cols + 1) * 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for fn in (Q.quotient_dev, Q.cosets_dev):
            fn(ctx, d_small, 1, 2, cols, prog, s, s_inv, d_tmp, d_tmp.data_ptr() + 32 * cols * 8)
        ctx.sync()
        ctx.close()
        for log, e in [tuple(int(v) for v in x.split(":")) for x in a.shapes.split(",")]:
            k, n, n_ext = log - e, 1 << (log - e), 1 << log
            d_coeffs = device_scalars(torch, cols * n, 7000 + log)
            d_work_q = torch.empty(32 * cols * n_ext, dtype=torch.uint8, device="cuda")
            d_work_c = torch.empty(32 * cols * n, dtype=torch.uint8, device="cuda")
            d_h_q = torch.empty(32 * n_ext, dtype=torch.uint8, device="cuda")
            d_h_c = torch.empty(32 * n_ext, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            routes = []
            for fn, d_work, d_h in ((Q.quotient_dev, d_work_q, d_h_q), (Q.cosets_dev, d_work_c, d_h_c)):
                ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
                ctx.sync()
                call = (lambda fn=fn, ctx=ctx, d_work=d_work, d_h=d_h: fn(ctx, d_coeffs, k, e, cols, prog, s, s_inv, d_work, d_h))
                torch.cuda.synchronize()
                free_before = torch.cuda.mem_get_info()[0]
                call()  # the first call of the shape: the slots grow
                ctx.sync()
                torch.cuda.synchronize()
                grew = free_before - torch.cuda.mem_get_info()[0]
                routes.append((ctx, call, grew, []))
            for i in range(WARMUPS + RUNS):
                for ctx, call, _, ts in routes:
                    t0 = time.perf_counter()
                    call()
                    ctx.sync()
                    if i >= WARMUPS:
                        ts.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            same = torch.equal(d_h_q, d_h_c)
            (_, _, grew_q, t_q), (_, _, grew_c, t_c) = routes
            lines.append("%-7s %3d %2d   %s   %s   %10.2f   %9.1f  %12.1f  %9.1f  %10.1f   %s" % (
                curve, log, e, fmt(t_q), fmt(t_c), statistics.median(t_c) / statistics.median(t_q),
                32 * (cols + 1) * n_ext / MIB, 32 * (cols * n + n_ext) / MIB, grew_q / MIB, grew_c / MIB,
                "equal byte for byte" if same else "DIFFERENT"))
            print(lines[-1], flush=True)
            for ctx, _, _, _ in routes:
                ctx.close()
            del routes, d_coeffs, d_work_q, d_work_c, d_h_q, d_h_c
            torch.cuda.empty_cache()
            assert same, "the two routes wrote different bytes"
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
