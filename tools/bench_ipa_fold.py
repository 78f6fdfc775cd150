#!/usr/bin/env python3
"""`decide_all` over m accumulators: `snarkv_ipa_decide_batch` (m MSMs of 2^k terms) against `snarkv_ipa_decide_folded`
(one MSM of 2^k terms and one of m terms over a random linear combination; csrc/ipa_fold.hip), both curves.

Routes, one worker process each:
  batch       snarkv_ipa_decide_batch of this build, the key's window table prepared beforehand where it fits
  folded      snarkv_ipa_decide_folded on a key without a table
  folded_tbl  the same on a key whose table was prepared (it serves the 2^k-term MSM up to k = 14)
The workers of a curve stay alive side by side and take turns, call by call, so drift of the machine falls on all
routes alike.  Every call ends synchronised (the verdict is back on the host): a host clock around the call is the
measurement; 3 warm-ups, then the median of --reps rounds with [min .. max].  Every U is a point of the curve (an
off-curve one would end the folded call at its validation); the verdict is not what is timed.  The kernels' own times
come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_ipa_fold.py --single CURVE --shape K,M`.

    python tools/bench_ipa_fold.py [--reps 11] [--k 8,11,14,16,18] [--m 1,4,64,1024] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ipa_batch import Bench, R, M_1024_MAX_K, ask  # noqa: E402

ROUTES = ["batch", "folded", "folded_tbl"]


class FoldBench(Bench):
    def __init__(self, curve, route):
        super().__init__(curve)
        self.route = route
        self.rho = self.rnd.randrange(R[curve]).to_bytes(32, "little")

    def key(self, k):
        fresh = k not in self.keys
        out = super().key(k)
        if fresh and self.route != "folded":
            out[0].prepare()  # a no-op for a key whose table would not fit
        return out

    def call_ms(self, k, m, xi, u):
        dk = self.key(k)[0]
        t0 = time.perf_counter()
        if self.route == "batch":
            self.ctx.ipa_decide_batch(dk, xi, u)
        else:
            self.ctx.ipa_decide_folded(dk, xi, u, self.rho)
        return (time.perf_counter() - t0) * 1e3


def worker(curve, route):
    b = FoldBench(curve, route)
    cache = {}
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        k, m = int(cmd[1]), int(cmd[2])
        if (k, m) not in cache:
            cache.clear()
            cache[(k, m)] = b.inputs(k, m)
        print("%.4f" % b.call_ms(k, m, *cache[(k, m)]), flush=True)


def single(curve, shape):
    """the folded route in one process, for a kernel trace: 3 warm-ups and 10 calls at one shape; prints the host's median"""
    k, m = shape
    b = FoldBench(curve, "folded")
    xi, u = b.inputs(k, m)
    t = [b.call_ms(k, m, xi, u) for _ in range(13)][3:]
    print("single %s k=%d m=%d folded %.3f ms per call (median of 10, host clock, under the profiler)" % (curve, k, m, statistics.median(t)))


def spawn(curve, route):
    env = dict(os.environ)
    env.pop("SNARKV_IPA_SHARED", None)
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", curve, "--route", route], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, env=env)
    assert p.stdout.readline().strip() == "ready", (curve, route)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default="")
    ap.add_argument("--route", default="folded")
    ap.add_argument("--single", default="")
    ap.add_argument("--shape", default="16,64")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--k", default="8,11,14,16,18")
    ap.add_argument("--m", default="1,4,64,1024")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.route)
    if a.single:
        return single(a.single, tuple(int(x) for x in a.shape.split(",")))
    ks, ms = [int(x) for x in a.k.split(",")], [int(x) for x in a.m.split(",")]
    lines = ["# tools/bench_ipa_fold.py: decide_all over m accumulators, ms per call: median [min .. max] of %d after 3 warm-ups,"
             % a.reps, "# routes alternating call by call; routes: " + ", ".join(ROUTES)]
    result, slower = {}, []
    for curve in a.curves.split(","):
        procs = {r: spawn(curve, r) for r in ROUTES}
        for k in ks:
            for m in ms:
                if m >= 1024 and k > M_1024_MAX_K:
                    continue
                t = {r: [] for r in ROUTES}
                for rep in range(3 + a.reps):
                    for r in ROUTES:
                        dt = ask(procs[r], "run", k, m)
                        if rep >= 3:
                            t[r].append(dt)
                row = {r: (statistics.median(v), min(v), max(v)) for r, v in t.items()}
                result["%s/%d/%d" % (curve, k, m)] = {r: list(v) for r, v in row.items()}
                lines.append("%s k = %2d m = %4d  " % (curve, k, m)
                             + "   ".join("%s %9.3f [%9.3f .. %9.3f]" % ((r,) + row[r]) for r in ROUTES)
                             + "   batch / folded %6.2f" % (row["batch"][0] / row["folded"][0]))
                for r in ROUTES[1:]:
                    if row[r][1] >= row["batch"][2]:
                        slower.append("%s wholly above batch at %s k=%d m=%d" % (r, curve, k, m))
                    elif row[r][0] >= row["batch"][0]:
                        slower.append("%s not faster than batch (medians; the ranges overlap) at %s k=%d m=%d" % (r, curve, k, m))
        for p in procs.values():
            p.stdin.write("quit\n")
            p.stdin.flush()
            p.wait(timeout=60)
    lines += ["# grid points where a folded route is not faster than batch"] + (slower or ["(none)"])
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bench": "ipa_fold", "ms": result}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
