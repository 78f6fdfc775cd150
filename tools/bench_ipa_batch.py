#!/usr/bin/env python3
"""`snarkv_ipa_decide_batch` over m accumulators: the per-accumulator Pippengers against the shared-key MSM over the
key's window table (csrc/msm_shared.hip), both curves.

Routes (the knob SNARKV_IPA_SHARED is read once per process, so every route is a worker process of its own):
  parent   the libraries of another build (--parent-libs DIR holding libsnarkv_amd.so and libsnarkv_pallas.so)
  pervec   this build, SNARKV_IPA_SHARED=0
  shared   this build, SNARKV_IPA_SHARED=1
  auto     this build, the knob unset: the thresholds of csrc/ipa.hip
The workers of a curve stay alive side by side and take turns, call by call, so drift of the machine falls on all
routes alike.  Every call ends synchronised (the verdicts are back on the host): a host clock around the call is the
measurement; 3 warm-ups, then the median of --reps rounds with [min .. max].  The table build (`prepare()` on a fresh key)
is timed apart, once per key size.  The kernels' own times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_ipa_batch.py --single CURVE`.

    python tools/bench_ipa_batch.py [--parent-libs DIR] [--reps 11] [--k 8,11,14,16] [--m 1,4,64,1024] [--out FILE]
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

R = {"bn254": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
     "pallas": 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001}
M_1024_MAX_K = 11  # m = 1 024 only up to this key size


class Bench:
    """one curve in this process: keys by size, one timed call at a time"""

    def __init__(self, curve):
        self.curve, self.keys, self.rnd = curve, {}, random.Random("ipa-batch-" + curve)
        if curve == "bn254":
            import snark_verifier_amd as sv

            self.sv, self.ctx = sv, sv.Context(0)
        else:
            from snark_verifier_amd import pallas as PL

            self.ctx = PL.PallasContext(0)

    def key_bytes(self, k):
        """2^k points s_i G: one segmented launch of single-term MSMs (no host curve arithmetic)"""
        n, r = 1 << k, R[self.curve]
        gen = (1).to_bytes(32, "little") + (2).to_bytes(32, "little") if self.curve == "bn254" else \
            ((1 << 254) + 45560315531419706090280762371685220353 - 1).to_bytes(32, "little") + (2).to_bytes(32, "little")
        s = b"".join(self.rnd.randrange(1, r).to_bytes(32, "little") for _ in range(n))
        return self.ctx.msm_batched(s, gen * n, list(range(n + 1)))

    def key(self, k):
        if k not in self.keys:
            gb = self.key_bytes(k)
            if self.curve == "bn254":
                mk = lambda: self.sv.IpaDecidingKey(self.ctx, gb)  # noqa: E731
            else:
                mk = lambda: self.ctx.ipa_dk_create(gb)  # noqa: E731
            self.keys[k] = (mk(), gb, mk)
        return self.keys[k]

    def build_ms(self, k):
        """`prepare()` on a fresh handle of the key (0.0 when this build has no table or the knob forbids it)"""
        _, _, mk = self.key(k)
        dk = mk()
        if not hasattr(dk, "prepare") or os.environ.get("SNARKV_IPA_SHARED") == "0":
            dk.close()
            return 0.0
        t0 = time.perf_counter()
        dk.prepare()
        dt = (time.perf_counter() - t0) * 1e3
        assert dk.table_bytes == 32 * (1 << k) * 64
        dk.close()
        return dt

    def inputs(self, k, m):
        r = R[self.curve]
        xi = b"".join(self.rnd.randrange(r).to_bytes(32, "little") for _ in range(k * m))
        return xi, self.key(k)[1][:64] * m  # any point: the verdict is not what is timed

    def call_ms(self, k, m, xi, u):
        dk = self.key(k)[0]
        t0 = time.perf_counter()
        self.ctx.ipa_decide_batch(dk, xi, u)
        return (time.perf_counter() - t0) * 1e3


def worker(curve):
    b = Bench(curve)
    cache = {}
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        k = int(cmd[1])
        if cmd[0] == "build":
            print("%.4f" % b.build_ms(k), flush=True)
        else:
            m = int(cmd[2])
            if (k, m) not in cache:
                cache.clear()
                cache[(k, m)] = b.inputs(k, m)
            print("%.4f" % b.call_ms(k, m, *cache[(k, m)]), flush=True)


def single(curve):
    """the shared route in one process, for a kernel trace: a few calls at the two shapes the record quotes"""
    b = Bench(curve)
    for k, m in ((8, 1024), (14, 64)):
        b.key(k)[0].prepare()
        xi, u = b.inputs(k, m)
        for _ in range(5):
            b.call_ms(k, m, xi, u)


def spawn(curve, route, parent_libs):
    env = dict(os.environ)
    env.pop("SNARKV_IPA_SHARED", None)
    if route == "parent":
        env["SNARKV_AMD_LIB"] = os.path.join(parent_libs, "libsnarkv_amd.so")
        env["SNARKV_PALLAS_LIB"] = os.path.join(parent_libs, "libsnarkv_pallas.so")
    elif route != "auto":
        env["SNARKV_IPA_SHARED"] = "0" if route == "pervec" else "1"
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", curve], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, env=env)
    assert p.stdout.readline().strip() == "ready", (curve, route)
    return p


def ask(p, *cmd):
    p.stdin.write(" ".join(str(c) for c in cmd) + "\n")
    p.stdin.flush()
    return float(p.stdout.readline())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default="")
    ap.add_argument("--single", default="")
    ap.add_argument("--parent-libs", default="")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--k", default="8,11,14,16")
    ap.add_argument("--m", default="1,4,64,1024")
    ap.add_argument("--curves", default="bn254,pallas")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if a.single:
        return single(a.single)
    routes = (["parent"] if a.parent_libs else []) + ["pervec", "shared", "auto"]
    base = routes[0]  # what auto and shared are held against
    ks, ms = [int(x) for x in a.k.split(",")], [int(x) for x in a.m.split(",")]
    lines = ["# tools/bench_ipa_batch.py: snarkv_ipa_decide_batch, ms per call: median [min .. max] of %d after 3 warm-ups,"
             % a.reps, "# routes alternating call by call; routes: " + ", ".join(routes)]
    result, verdicts = {}, []
    for curve in a.curves.split(","):
        procs = {r: spawn(curve, r, a.parent_libs) for r in routes}
        for k in ks:
            lines.append("%s k = %2d  table build (prepare on a fresh key): %8.2f ms, %d KiB"
                         % (curve, k, ask(procs["shared"], "build", k), 2 << k))
            for m in ms:
                if m >= 1024 and k > M_1024_MAX_K:
                    continue
                t = {r: [] for r in routes}
                for rep in range(3 + a.reps):
                    for r in routes:
                        dt = ask(procs[r], "run", k, m)
                        if rep >= 3:
                            t[r].append(dt)
                row = {r: (statistics.median(v), min(v), max(v)) for r, v in t.items()}
                result["%s/%d/%d" % (curve, k, m)] = {r: list(v) for r, v in row.items()}
                lines.append("%s k = %2d m = %4d  " % (curve, k, m)
                             + "   ".join("%s %9.3f [%9.3f .. %9.3f]" % ((r,) + row[r]) for r in routes))
                spread = row[base][2] - row[base][1]
                if row["auto"][0] > row[base][0] + spread:
                    verdicts.append("MISS auto slower than %s beyond its spread at %s k=%d m=%d" % (base, curve, k, m))
                if (k, m) == (8, 1024):
                    ok = row["shared"][2] < row[base][1]
                    verdicts.append("%s shared range %s %s's at %s k=8 m=1024" % ("OK  " if ok else "MISS", "wholly below" if ok else "not below", base, curve))
        for p in procs.values():
            p.stdin.write("quit\n")
            p.stdin.flush()
            p.wait(timeout=60)
    lines += ["# checks"] + (verdicts or ["(none)"])
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bench": "ipa_batch", "base": base, "ms": result}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
