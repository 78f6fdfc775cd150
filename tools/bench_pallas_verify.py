#!/usr/bin/env python3
"""Batch verification of halo2 IPA proofs on pallas: who should take the square roots?

64 seeded PLONK-over-IPA proofs at k = 8 (28 compressed points each), replicated to N = 64 / 256 / 1024, read and
succinct-verified through
  (a) hooks    `hp_plonk_ipa_verify_batch` with decide = 0: the only route before the product API (proofs read on one
               thread, the key re-parsed on every call)
  (b) host     snarkv_host_pallas_plonk_succinct_verify_batch, SNARKV_HOST_PALLAS_DECOMPRESS_HOST
  (c) device   the same entry point, SNARKV_HOST_PALLAS_DECOMPRESS_DEVICE
  (d) verify   snarkv_host_pallas_plonk_verify, DEVICE decompression: the succinct half of (c) AND `decide_all` over the N
               accumulators (one process per setting of SNARKV_IPA_SHARED: the knob is read once; not in the default set)
with 16 host threads.  The routes alternate inside one process; every call ends synchronised (the accumulators are
back on the host), so a host clock around the call is the measurement: 3 warm-ups, then the median of --reps rounds,
with min / max as the spread.  The kernel's own time comes from a separate run of this tool with `--routes c` under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR`; `--kernel-trace DIR` then prints the launches of
`k_g1_decompress` found in DIR by batch size.

    python tools/bench_pallas_verify.py [--proofs FILE] [--reps 11] [--n 64,256,1024] [--routes a,b,c] [--out FILE]
    python tools/bench_pallas_verify.py --kernel-trace DIR [--n 64,256,1024] [--out FILE]

--proofs FILE: the forged proofs are written there on the first run and read back later (forging is pure Python)."""
import argparse
import ctypes
import json
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, BASE, THREADS = 8, 64, 16


def forge(path):
    if path and os.path.exists(path):
        with open(path) as f:
            d = json.load(f)
        return {k: bytes.fromhex(v) if isinstance(v, str) else [bytes.fromhex(x) for x in v] for k, v in d.items()}
    import hostfmt
    import pallas as PA
    import plonk as P
    import plonk_synth as S
    import transcript as T

    S.use_curve(PA)
    hostfmt.use_curve(PA)
    rng = random.Random("bench-pallas-verify")
    pr, dl = S.standard_plonk_protocol(rng, k=K, num_instance=(3,))
    kd = {"g": [rng.randrange(1, PA.R) for _ in range(1 << K)], "h": rng.randrange(1, PA.R), "s": rng.randrange(1, PA.R)}
    g = [PA.g1_mul(PA.G1_GEN, c) for c in kd["g"]]
    mk = lambda stream=b"": T.Blake2bTranscript(PA, stream)  # noqa: E731
    insts = [[[rng.randrange(PA.R) for _ in range(3)]] for _ in range(BASE)]
    d = {"protocol": S.pack_protocol(pr), "g": b"".join(PA.g1_to_bytes(p) for p in g),
         "h": PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, kd["h"])), "s": PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, kd["s"])),
         "instances": [S.pack_instances(x) for x in insts],
         "proofs": [P.forge_proof_ipa(pr, insts[i], kd, mk, rng, dl) for i in range(BASE)]}
    if path:
        with open(path, "w") as f:
            json.dump({k: v.hex() if isinstance(v, bytes) else [x.hex() for x in v] for k, v in d.items()}, f)
    return d


def kernel_trace(root, ns, out):
    """the launches of k_g1_decompress in a rocprofv3 CSV kernel trace, by launch size (one lane per point, workgroups of
    64): a batch of N proofs is the launch of ceil(N (12 + 2k) / 64) workgroups"""
    import csv

    by_grid = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(d, f)) as fh:
                    for r in csv.DictReader(fh):
                        if "k_g1_decompress" in r["Kernel_Name"]:
                            by_grid.setdefault(int(r.get("Grid_Size") or r["Grid_Size_X"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["# k_g1_decompress alone (rocprofv3 --kernel-trace, route c): us per launch, median [min .. max] over the launches"]
    for n in ns:
        lanes = n * (12 + 2 * K)
        t = by_grid.get((lanes + 63) // 64 * 64, [])
        if t:
            lines.append("N = %4d  %6d points  %4d wavefronts  %3d launches  %8.1f [%8.1f .. %8.1f]"
                         % (n, lanes, (lanes + 63) // 64, len(t), statistics.median(t), min(t), max(t)))
        else:
            lines.append("N = %4d  no launch of %d lanes in the trace (sizes seen: %s)" % (n, (lanes + 63) // 64 * 64, sorted(by_grid)))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-trace", default="")
    ap.add_argument("--proofs", default="")
    ap.add_argument("--forge-only", action="store_true")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--n", default="64,256,1024")
    ap.add_argument("--routes", default="a,b,c")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.kernel_trace:
        return kernel_trace(a.kernel_trace, [int(x) for x in a.n.split(",")], a.out)
    d = forge(a.proofs)
    if a.forge_only:
        return
    assert len(d["proofs"][0]) == 32 * (12 + 2 * K + 25)

    import importlib.util

    from snark_verifier_amd import host_api_pallas as H
    from snark_verifier_amd import pallas as PL

    PL.load_library()
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    hooks = ctypes.CDLL(b.build_host_driver_pallas())
    fn = hooks.hp_plonk_ipa_verify_batch
    fn.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                   ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint,
                   ctypes.c_char_p, ctypes.c_int]
    H.load_library()
    protocol = H.Protocol(d["protocol"])
    dk = H.IpaDecidingKey(K, d["g"], d["h"], d["s"])
    svk = struct.pack("<II", K, 1) + d["g"][:64] + d["h"] + d["s"]
    routes = a.routes.split(",")
    lines = ["# tools/bench_pallas_verify.py: k = %d, %d base proofs of %d bytes (%d points), host_threads = %d, reps = %d"
             % (K, BASE, len(d["proofs"][0]), 12 + 2 * K, THREADS, a.reps),
             "# ms per call: median [min .. max];  a = hooks (decide = 0), b = API HOST, c = API DEVICE, d = plonk_verify (c + decide_all)",
             "# SNARKV_IPA_SHARED = %s" % os.environ.get("SNARKV_IPA_SHARED", "unset")]
    result = {}
    for n in [int(x) for x in a.n.split(",")]:
        ib = b"".join(d["instances"][i % BASE] for i in range(n))
        pb = H.pack_proofs([d["proofs"][i % BASE] for i in range(n)])
        stride = 32 * K + 64
        out = ctypes.create_string_buffer(stride * n)

        def run(route):
            t0 = time.perf_counter()
            if route == "d":
                ok = H.plonk_verify(protocol, dk, ib, pb, n, THREADS, H.DECOMPRESS_DEVICE)
                assert ok, route
                return (time.perf_counter() - t0) * 1e3, None
            if route == "a":
                rc = fn(2, d["protocol"], len(d["protocol"]), ib, len(ib), pb, len(pb), n, svk, d["g"], 1 << K, THREADS, out, 0)
                accs = out.raw
            else:
                rc, accs = H.plonk_succinct_verify_batch(protocol, dk, ib, pb, n, THREADS,
                                                         H.DECOMPRESS_HOST if route == "b" else H.DECOMPRESS_DEVICE)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 1, (route, rc)
            return dt, accs

        times = {r: [] for r in routes}
        ref = None
        for rep in range(3 + a.reps):
            for r in routes:  # the routes alternate: drift of the machine falls on all of them alike
                dt, accs = run(r)
                if ref is None and accs is not None:
                    ref = accs
                assert accs is None or accs == ref, "route %s disagrees" % r
                if rep >= 3:
                    times[r].append(dt)
        row = {r: (statistics.median(t), min(t), max(t)) for r, t in times.items()}
        result[n] = row
        lines.append("N = %4d  " % n + "   ".join("%s %8.2f [%8.2f .. %8.2f]" % ((r,) + row[r]) for r in routes))
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"bench": "pallas_verify", "k": K, "host_threads": THREADS,
                      "ms": {str(n): {r: v[0] for r, v in row.items()} for n, row in result.items()}}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    dk.close()
    protocol.close()


if __name__ == "__main__":
    main()
