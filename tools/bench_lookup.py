"""Times the lookup calls (snark_verifier_amd.lookup, columns resident on the device) on BN254 and pallas at 2^10, 2^16, 2^20
and 2^24 rows: `sort_dev`, `permute_dev` and `product_dev`, each on two kinds of input --

  uniform   the table is uniform in [0, 2^252), the input a shuffle of it (a theta-compressed lookup)
  range     the table is the integers below 2^16 (below n where n is smaller), repeated to n rows and shuffled, the input
            uniform among them (a single-column range lookup: small keys, long ties)

-- next to yardsticks taken in the same process:

  (a) a device-to-device copy of one column (n x 32 bytes) times the columns the call reads and writes: sort 2, permute 4,
      product 5;
  (b) one forward transform of that size (`ntt.ntt_dev`);
  (c) for `product_dev`: a `poly_prod.perm_product_dev` of one column set (value, identity, sigma) of the same n.

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise).

    python tools/bench_lookup.py [--logs 10,16,20,24] [--curves bn254,pallas] [--out FILE]

`/copy` is the call's time over the copies, `/ntt` over the transform, `/perm` over (c).  The sort is timed out of place on
unsorted input every time; the permuted columns that the product reads come from `permute_dev`, and its status is asserted
zero.  Nothing routes on these numbers and none is a pass mark."""
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
RANGE_LOG = 16


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


def small_scalars(torch, values):
    """int64 values below 2^63 -> 32-byte little-endian elements"""
    t = torch.zeros((values.numel(), 32), dtype=torch.uint8, device="cuda")
    for b in range(8):
        t[:, b] = ((values >> (8 * b)) & 0xFF).to(torch.uint8)
    return t.reshape(-1)


def inputs(torch, kind, n, seed):
    """-> (input column, table column), n elements each, on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if kind == "uniform":
        table = device_scalars(torch, n, seed).reshape(n, 32)
        return table[torch.randperm(n, device="cuda", generator=g)].reshape(-1).contiguous(), table.reshape(-1)
    m = min(n, 1 << RANGE_LOG)
    table = (torch.arange(n, device="cuda") % m)[torch.randperm(n, device="cuda", generator=g)]
    return small_scalars(torch, torch.randint(0, m, (n,), device="cuda", generator=g)), small_scalars(torch, table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="10,16,20,24")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import lookup as L
    from snark_verifier_amd import ntt as N
    from snark_verifier_amd import pallas as PL
    from snark_verifier_amd import poly_prod as P

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max]" % (RUNS, WARMUPS),
             "# n = 2^log rows; copy: device-to-device copy of one column x the columns the call reads and writes;",
             "# ntt: one forward transform of 2^log; perm: poly_perm_product_dev of one column set of the same n",
             "# curve  log  input    call      cols   call                               copy x cols                        "
             "ntt                                  /copy    /ntt   /perm"]
    beta, gamma = 0x1234567 << 100 | 5, 0x7654321 << 90 | 3
    for curve in a.curves.split(","):
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        for log in [int(x) for x in a.logs.split(",")]:
            n = 1 << log
            d_tmp = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
            d_polys = torch.empty(32 * 4 * n, dtype=torch.uint8, device="cuda")  # A, S, A', S'
            d_work = torch.empty(32 * 2 * n, dtype=torch.uint8, device="cuda")
            d_z = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
            d_small = torch.zeros(64, dtype=torch.uint8, device="cuda")  # the status, then a total
            col = lambda j: d_polys.data_ptr() + 32 * n * j  # noqa: E731
            for kind in ("uniform", "range"):
                d_a, d_s = inputs(torch, kind, n, 7000 + log)
                d_polys[:32 * n] = d_a
                d_polys[32 * n:64 * n] = d_s
                torch.cuda.synchronize()
                t_once = timed(lambda: d_tmp.copy_(d_z), torch.cuda.synchronize)
                t_ntt = timed(lambda: N.ntt_dev(ctx, d_z, d_tmp, log), ctx.sync)
                # one column set of the permutation argument over the same columns: value A, identity S, sigma A
                t_perm = timed(lambda: P.perm_product_dev(ctx, d_polys, n, 2, [0], [1], [0], beta, gamma, d_work, d_z), ctx.sync)
                L.permute_dev(ctx, col(0), col(1), n, d_work, col(2), col(3), d_small)
                ctx.sync()
                assert bytes(d_small[:4].cpu().numpy()) == bytes(4), "the lookup is satisfied"
                calls = (
                    ("sort", 2, lambda: L.sort_dev(ctx, col(0), n, d_work, d_z)),
                    ("permute", 4, lambda: L.permute_dev(ctx, col(0), col(1), n, d_work, col(2), col(3), d_small)),
                    ("product", 5, lambda: L.product_dev(ctx, d_polys, n, 4, 0, 1, 2, 3, beta, gamma, d_work, d_z,
                                                         d_total=d_small.data_ptr() + 32)),
                )
                for name, width, fn in calls:
                    t = timed(fn, ctx.sync)
                    t_copy = tuple(width * x for x in t_once)
                    lines.append("%-7s %3d  %-8s %-8s %5d   %s   %s   %s   %7.2f %7.2f %7s" % (
                        curve, log, kind, name, width, fmt(t), fmt(t_copy), fmt(t_ntt), t[0] / t_copy[0], t[0] / t_ntt[0],
                        "%7.2f" % (t[0] / t_perm[0]) if name == "product" else "-"))
                    print(lines[-1], flush=True)
                    if name == "product":
                        assert bytes(d_small[32:64].cpu().numpy()) == (1).to_bytes(32, "little"), "the product closes"
                        lines.append("%-7s %3d  %-8s %-8s %5d   %s" % (curve, log, kind, "perm", 5, fmt(t_perm)))
                        print(lines[-1], flush=True)
                del d_a, d_s
            del d_tmp, d_polys, d_work, d_z, d_small
        ctx.close()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
