"""Times the inverse transform over group elements (snark_verifier_amd.g1_ntt.intt_dev: a key's points to its Lagrange basis)
at k = 10, 16, 20, two legs alternating in one process:

  bn254   the transform against the same transform composed of k calls of `snarkv_g1_msm_batched_dev`, n two-term MSMs per
          pass (out = c a + c w^-e b, c = 1 or, in the last pass, n^-1).  The composition's scalars and gather indices are
          made before the clock starts; inside it are, per pass, the gather of the 2n points (torch), the call, and the two
          synchronisations that order torch's stream and the context's.  The tool asserts equal bytes at every k.
  pallas  the transform alone (its library has no device-resident batched MSM); equal bytes are asserted at k = 12 against the
          composition through the host-staged `snarkv_pallas_g1_msm_batched`.

3 warm-ups, then the median of 11 with [min .. max], ms on the host clock (call + synchronise).

    python tools/bench_g1_ntt.py [--ks 10,16,20] [--curves bn254,pallas] [--out FILE]

The composition multiplies twice per butterfly (both outputs), the transform once.  Nothing routes on these numbers."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WARMUPS, RUNS = 3, 11
PALLAS_CHECK_K = 12


def fmt(t):
    return "%10.3f [%10.3f .. %10.3f]" % t


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def timed_alternating(legs, sync):
    """legs: name -> fn; every round runs each leg once, in turn"""
    ts = {name: [] for name in legs}
    for i in range(WARMUPS + RUNS):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= WARMUPS:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: stats(v) for name, v in ts.items()}


class Composition:
    """the inverse transform as k launches of n two-term MSMs: per pass the indices of the points (a, b of every output) and
    the scalars (c, c w^-x), the powers taken from the scalar transforms of the unit vector e_1"""

    def __init__(self, torch, ctx, k):
        from snark_verifier_amd import ntt as N

        self.torch, self.ctx, self.k, n = torch, ctx, k, 1 << k
        e1 = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        e1[1, 0] = 1
        fwd, inv = torch.empty_like(e1), torch.empty_like(e1)  # w^i and n^-1 w^-i
        torch.cuda.synchronize()
        N.ntt_dev(ctx, e1, fwd, k)
        N.intt_dev(ctx, e1, inv, k)
        ctx.sync()
        m = torch.arange(n, dtype=torch.int64, device="cuda")
        self.point_idx, self.scalars = [], []
        for s in range(k):
            kk, hi = m & ((1 << s) - 1), (m >> s) & 1
            j = ((m >> (s + 1)) << s) + kk
            x = (kk << (k - 1 - s)) + hi * (n // 2)  # a - t = a + w^-(e + n/2) b
            last = s == k - 1
            table, at = (inv, x) if last else (fwd, (n - x) % n)
            self.point_idx.append(torch.stack([j, j + n // 2], dim=1).reshape(-1))
            self.scalars.append(torch.stack([table[0].expand(n, 32), table.index_select(0, at)], dim=1).reshape(-1).contiguous())
        self.offsets = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device="cuda")
        self.work = [torch.empty((n, 64), dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()

    def run_dev(self, d_in):
        """-> the tensor that holds the result (one of the two working buffers); the context is synchronised"""
        torch, n = self.torch, 1 << self.k
        src = d_in.view(n, 64)
        for s in range(self.k):
            pts = src.index_select(0, self.point_idx[s])
            torch.cuda.synchronize()
            self.ctx.msm_batched_dev(self.scalars[s].data_ptr(), pts.data_ptr(), self.offsets.data_ptr(), n, 2 * n,
                                     self.work[s & 1].data_ptr())
            self.ctx.sync()
            src = self.work[s & 1]
        return src

    def run_host_staged(self, d_in):
        """the same through the host-staged batched MSM -> bytes"""
        n = 1 << self.k
        src = d_in.view(n, 64)
        offs = list(range(0, 2 * n + 1, 2))
        for s in range(self.k):
            pts = src.index_select(0, self.point_idx[s]).cpu().numpy().tobytes()
            raw = self.ctx.msm_batched(self.scalars[s].cpu().numpy().tobytes(), pts, offs)
            src = self.torch.frombuffer(bytearray(raw), dtype=self.torch.uint8).cuda().view(n, 64)
        return src.cpu().numpy().tobytes()


def points(torch, G, ctx, curve, k):
    """2^k distinct points on the device"""
    n = 1 << k
    d = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    if curve == "bn254":
        torch.cuda.synchronize()
        ctx.sample_points_dev(100 + k, n, d.data_ptr())
    else:  # the forward transform of 64 sampled points and n - 64 identities: n combinations of them
        import pallas as PA

        seed = b"".join(PA.g1_to_bytes(p) for p in PA.sample_points(20, 64))
        d[:len(seed)] = torch.frombuffer(bytearray(seed), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        G.ntt_dev(ctx, d, d, k)
    ctx.sync()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="10,16,20")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd import g1_ntt as G
    from snark_verifier_amd import pallas as PL

    lines = ["# ms on the host clock (call + synchronise): median of %d after %d warm-ups [min .. max], the legs alternating" % (RUNS, WARMUPS),
             "# transform: g1_ntt.intt_dev of 2^k points; composed: the same as k launches of n two-term MSMs (snarkv_g1_msm_batched_dev),",
             "#   the gather of its points and two synchronisations per pass inside the clock, its scalars and indices outside",
             "# curve   k   transform                              composed                               composed / transform"]
    for curve in a.curves.split(","):
        ctx = sv.Context(0) if curve == "bn254" else PL.PallasContext(0)
        if curve == "pallas":
            k = PALLAS_CHECK_K
            d_in, d_out = points(torch, G, ctx, curve, k), torch.empty(64 << k, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            G.intt_dev(ctx, d_in, d_out, k)
            ctx.sync()
            assert d_out.cpu().numpy().tobytes() == Composition(torch, ctx, k).run_host_staged(d_in), "pallas: bytes differ at k = %d" % k
            lines.append("# pallas: equal bytes at k = %d against the composition through the host-staged batched MSM" % k)
            print(lines[-1], flush=True)
        for k in [int(x) for x in a.ks.split(",")]:
            d_in, d_out = points(torch, G, ctx, curve, k), torch.empty(64 << k, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            legs = {"transform": lambda: G.intt_dev(ctx, d_in, d_out, k)}
            if curve == "bn254":
                comp = Composition(torch, ctx, k)
                legs["composed"] = lambda: comp.run_dev(d_in)
            t = timed_alternating(legs, ctx.sync)
            if curve == "bn254":
                assert torch.equal(comp.run_dev(d_in).reshape(-1), d_out), "bn254: bytes differ at k = %d" % k
                lines.append("%-7s %3d   %s   %s   %6.2f" % (curve, k, fmt(t["transform"]), fmt(t["composed"]),
                                                             t["composed"][0] / t["transform"][0]))
                del comp
            else:
                lines.append("%-7s %3d   %s" % (curve, k, fmt(t["transform"])))
            print(lines[-1], flush=True)
            del d_in, d_out
        ctx.close()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
