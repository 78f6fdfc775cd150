"""Builds libsnarkv_amd.so (HIP kernels + C ABI) for gfx950, in-tree.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU.  Objects land in
`snark-verifier_amd/build/`, the shared library next to this file so it travels
with the gpurun snapshot.  Rebuilds only what is stale.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libsnarkv_amd.so")
UNITS = ["ctx", "msm_api", "capi", "msm_naive", "msm_pippenger", "decider", "sample", "poseidon", "ipa", "ipa_prover", "mgpu",
         "decompress", "msm_shared", "ipa_fold", "ipa_opening", "ipa_create", "poly", "ipa_multiopen", "ntt",
         "poly_prod", "quotient", "lookup", "poly_batch", "kzg_multiopen", "plonk_prove", "g1_ntt"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result"]
FLAGS += os.environ.get("SNARKV_EXTRA_FLAGS", "").split()


# the public headers the device units include (include/; the host mirror's are in _host_stale)
DEVICE_HEADERS = ("amd", "pallas", "pallas_decompress", "ipa_prover", "ipa_batch", "ipa_fold", "ipa_create", "poly", "ipa_multiopen",
                  "ntt", "poly_prod", "quotient", "quotient_cosets", "lookup", "poly_batch", "kzg_multiopen", "plonk_prove",
                  "ipa_commit_blinded", "pallas_session", "g1_ntt")


def _deps():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".inc"))]
    hdrs += [os.path.join(HERE, "..", "include", "snarkv_%s.h" % h) for h in DEVICE_HEADERS]
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(unit, verbose, extra=(), tag=""):
    src = os.path.join(CSRC, unit + ".hip")
    obj = os.path.join(BUILD, unit + tag + ".o")
    newest = max(os.path.getmtime(src), _deps())
    if os.path.exists(obj) and os.path.getmtime(obj) >= newest:
        return obj, False
    cmd = [HIPCC] + FLAGS + list(extra) + ["-c", src, "-o", obj]
    if verbose:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, capture_output=True, text=True)
    with open(os.path.join(BUILD, unit + tag + ".log"), "w") as f:
        f.write(r.stdout + r.stderr)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for %s" % unit)
    return obj, True


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    # every unit of both libraries in one pool (hipcc is single-threaded per unit)
    jobs = [(u, (), "") for u in UNITS] + [(u, tuple(PALLAS_FLAGS), "_pallas") for u in PALLAS_UNITS]
    with ThreadPoolExecutor(max_workers=min(len(jobs) + len(DEVTEST_FLAVOURS), os.cpu_count() or 4)) as ex:
        devtest = [ex.submit(build_devtest, f) for f in DEVTEST_FLAVOURS]  # the test-only device units ride in the same pool
        devtest += [ex.submit(build_hosttest, n, c) for n in HOSTTESTS for c in ("bn254", "pallas")]
        res = list(ex.map(lambda j: _compile(j[0], verbose, j[1], j[2]), jobs))
        for d in devtest:
            d.result()
    _link(LIB, res[:len(UNITS)], [])
    _link(PALLAS_LIB, res[len(UNITS):], ["-Wl,-Bsymbolic"])  # its internals never bind by symbol lookup across libraries
    build_host_driver()
    return LIB


def _link(lib, res, extra):
    if any(ch for _, ch in res) or not os.path.exists(lib):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + extra + ["-o", lib] + [o for o, _ in res]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError("link failed: %s" % os.path.basename(lib))


# The pasta build of the curve-generic units (csrc/pallas.hip explains the flags, csrc/ctx.hpp the policy they select).
PALLAS_UNITS = ["ctx", "msm_api", "pallas", "msm_pippenger", "msm_naive", "ipa", "ipa_prover", "decompress_pallas", "msm_shared",
                "ipa_fold", "ipa_opening", "ipa_create", "poly", "ipa_multiopen", "ntt", "poly_prod", "quotient", "lookup",
                "poly_batch", "session", "g1_ntt"]
PALLAS_FLAGS = ["-DSNARKV_CURVE_PALLAS", "-Dsnarkv=snarkv_pallas"]
PALLAS_LIB = os.path.join(HERE, "libsnarkv_pallas.so")


# Test-only device unit (tests/devtest/devtest.hip: one kernel per field / group operation, raw limbs in and out), in four
# flavours: both curves, each with the asm multiplier bodies and with the plain-C ones.  Compiled and linked in one step
# with the library's own FLAGS, next to its source, so that the artefacts travel with the tree like the libraries do.
DEVTEST_DIR = os.path.join(HERE, "..", "tests", "devtest")
DEVTEST_FLAVOURS = {"bn254_asm": [], "bn254_c": ["-DSNARKV_NO_SMAD_ASM"],
                    "pallas_asm": PALLAS_FLAGS, "pallas_c": PALLAS_FLAGS + ["-DSNARKV_NO_SMAD_ASM"]}


def devtest_sources():
    return [os.path.join(DEVTEST_DIR, "devtest.hip"), os.path.join(DEVTEST_DIR, "..", "hosttest", "curve_ops.h")]


# Host builds of the SNARKV_HD sources (tests/hosttest/hosttest_<name>.cpp), one library per curve, next to their source.
#   curve      the field and group operations of devtest.hip as plain C, the decider's rounds lane by lane
#   poly       the blocked scan of the polynomial division (csrc/poly_scan.h), the multi-open prover's query-set grouping
#   ntt        the transform (csrc/ntt_plan.h, csrc/ntt_tile.h)
#   poly_prod  the column products (csrc/poly_prod.h)
#   quotient   the gate program and the vanishing table (csrc/quotient.h)
#   lookup     the comparison, merge path, tiled sort and permute rule (csrc/lookup.h)
#   args       the entry points' shared argument checks (csrc/poly_args.hpp)
#   kzg_open   the host-side plan of the KZG multi-open provers (csrc/kzg_multiopen_plan.h)
#   quotient_cosets  the join of the coset-at-a-time quotient, tile by tile (csrc/quotient.h)
#   blind      the blind term of a blinded commitment, lane by lane and level by level (csrc/msm_blind.h)
#   curve_fm   the friendly-multiple products of csrc/fq29.h and the fast adders of csrc/g1_29.h on them, raw limbs
#   g1_ntt     the pass body of the transform over group elements, lane by lane and pass by pass (csrc/g1_ntt.h)
HOSTTEST_DIR = os.path.join(HERE, "..", "tests", "hosttest")
HOSTTESTS = ("curve", "poly", "ntt", "poly_prod", "quotient", "lookup", "args", "kzg_open", "quotient_cosets", "blind", "curve_fm",
             "g1_ntt")
HOSTTEST_EXCEPTIONS = {"curve": ("libhosttest_%s.so", ("curve_ops.h",))}  # the others: libhosttest_<name>_<curve>.so, one source


def build_hosttest(name, curve):
    stem, more = HOSTTEST_EXCEPTIONS.get(name, ("libhosttest_" + name + "_%s.so", ()))
    out = os.path.join(HOSTTEST_DIR, stem % curve)
    srcs = [os.path.join(HOSTTEST_DIR, f) for f in ("hosttest_%s.cpp" % name,) + more]
    if os.path.exists(out) and os.path.getmtime(out) >= max([_deps()] + [os.path.getmtime(f) for f in srcs]):
        return out
    flags = ["-DSNARKV_CURVE_PALLAS"] if curve == "pallas" else []
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", out, srcs[0]], capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("host build failed: hosttest_%s.cpp (%s)" % (name, curve))
    return out


def __getattr__(attr):
    """`build_hosttest_<name>(curve)` is `build_hosttest(name, curve)`: the spelling that callers outside this tree know"""
    name = attr[len("build_hosttest_"):]
    if attr.startswith("build_hosttest_") and name in HOSTTESTS:
        return lambda curve: build_hosttest(name, curve)
    raise AttributeError("module %r has no attribute %r" % (__name__, attr))


def devtest_lib(flavour):
    return os.path.join(DEVTEST_DIR, "libdevtest_%s.so" % flavour)


def build_devtest(flavour):
    out = devtest_lib(flavour)
    newest = max([_deps()] + [os.path.getmtime(f) for f in devtest_sources()])
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    cmd = [HIPCC] + FLAGS + DEVTEST_FLAVOURS[flavour] + ["-shared", "-Wl,-Bsymbolic", "-o", out, devtest_sources()[0]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for devtest %s" % flavour)
    return out


HOST = os.path.join(HERE, "host")
HOST_LIB = os.path.join(HERE, "libsnarkv_host.so")                 # product: C API of the host mirror (host/capi.cpp)
HOSTTEST_LIB = os.path.join(HERE, "libsnarkv_hosttest.so")         # test hooks only (host/test_driver.cpp)
HOST_PALLAS_LIB = os.path.join(HERE, "libsnarkv_hosttest_pallas.so")  # pasta flavour of the mirror, test hooks
HOST_PALLAS_API_LIB = os.path.join(HERE, "libsnarkv_host_pallas.so")  # pasta flavour, product C API (host/capi_pallas.cpp)
# the folded decide on top of it (host/capi_pallas_fold.cpp, include/snarkv_host_pallas_fold.h)
HOST_PALLAS_FOLD_LIB = os.path.join(HERE, "libsnarkv_host_pallas_fold.so")
# Ipa::create_proof in one call on top of it (host/capi_pallas_prove.cpp, include/snarkv_host_pallas_prove.h)
HOST_PALLAS_PROVE_LIB = os.path.join(HERE, "libsnarkv_host_pallas_prove.so")
# the PLONK prover session over IPA on top of it (host/capi_pallas_plonk_prove.cpp, include/snarkv_host_pallas_plonk_prove.h)
HOST_PALLAS_PLONK_PROVE_LIB = os.path.join(HERE, "libsnarkv_host_pallas_plonk_prove.so")
# ... and the same session with committed instances (host/capi_pallas_plonk_prove_ci.cpp, include/snarkv_host_pallas_plonk_prove_ci.h)
HOST_PALLAS_PLONK_PROVE_CI_LIB = os.path.join(HERE, "libsnarkv_host_pallas_plonk_prove_ci.so")


def _host_stale(out, dev_lib):
    inc = os.path.join(os.path.dirname(HERE), "include")
    srcs = [os.path.join(HOST, f) for f in os.listdir(HOST)] + [os.path.join(inc, h) for h in (
        "snarkv_host.h", "snarkv_host_pallas.h", "snarkv_pallas_decompress.h", "snarkv_host_pallas_fold.h", "snarkv_ipa_fold.h",
        "snarkv_host_pallas_prove.h", "snarkv_ipa_create.h", "snarkv_kzg_multiopen.h", "snarkv_host_kzg_open.h",
        "snarkv_host_plonk_prove.h", "snarkv_host_plonk_prove_opts.h", "snarkv_plonk_prove.h", "snarkv_quotient.h",
        "snarkv_quotient_cosets.h", "snarkv_ntt.h", "snarkv_poly.h", "snarkv_poly_batch.h", "snarkv_host_pallas_plonk_prove.h",
        "snarkv_pallas_session.h", "snarkv_ipa_multiopen.h", "snarkv_ipa_commit_blinded.h", "snarkv_host_pallas_plonk_prove_ci.h")]
    newest = max([os.path.getmtime(f) for f in srcs] + [os.path.getmtime(dev_lib)])
    return not os.path.exists(out) or os.path.getmtime(out) < newest


def _gxx(out, src, extra, dev, more_libs=()):
    # -mbmi2 -madx: mulx/adcx for the 4x64 Montgomery products (every x86-64 server CPU since 2015)
    cmd = ["g++", "-O3", "-mbmi2", "-madx", "-std=c++17", "-shared", "-fPIC"] + extra + ["-o", out, os.path.join(HOST, src),
           "-L" + HERE] + ["-l" + l for l in more_libs] + ["-l" + dev, "-pthread", "-Wl,-rpath,$ORIGIN"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("host build failed: %s" % src)
    return out


def build_host_driver():
    """C++ host mirror (host/*.hpp): its C API (host/capi.cpp -> libsnarkv_host.so, include/snarkv_host.h), the test
    hooks (host/test_driver.cpp -> libsnarkv_hosttest.so), and the pasta flavour's test hooks and C API
    (host/capi_pallas.cpp -> libsnarkv_host_pallas.so, include/snarkv_host_pallas.h), each linked against the
    device library next to it (rpath $ORIGIN).  Every target has its own staleness check."""
    jobs = []
    if _host_stale(HOST_LIB, LIB):
        jobs.append((HOST_LIB, "capi.cpp", [], "snarkv_amd"))
    if _host_stale(HOSTTEST_LIB, LIB):
        jobs.append((HOSTTEST_LIB, "test_driver.cpp", [], "snarkv_amd"))
    # -Dsnarkv_host=...: its own C++ namespace -- the two flavours define the same inline functions and
    # `static constexpr` members with different constants, and C++17 inline variables are STB_GNU_UNIQUE
    # (bound process-wide even under RTLD_LOCAL) when both libraries sit in one process
    pasta = ["-DSNARKV_HOST_PALLAS", "-Dsnarkv_host=snarkv_host_pallas", "-fno-gnu-unique"]
    if os.path.exists(PALLAS_LIB) and _host_stale(HOST_PALLAS_LIB, PALLAS_LIB):
        jobs.append((HOST_PALLAS_LIB, "test_driver_pallas.cpp", pasta, "snarkv_pallas"))
    if os.path.exists(PALLAS_LIB) and _host_stale(HOST_PALLAS_API_LIB, PALLAS_LIB):
        jobs.append((HOST_PALLAS_API_LIB, "capi_pallas.cpp", pasta, "snarkv_pallas"))
    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
            list(ex.map(lambda j: _gxx(*j), jobs))
    # links against the product library built above
    if os.path.exists(HOST_PALLAS_API_LIB) and _host_stale(HOST_PALLAS_FOLD_LIB, HOST_PALLAS_API_LIB):
        _gxx(HOST_PALLAS_FOLD_LIB, "capi_pallas_fold.cpp", pasta, "snarkv_pallas", ["snarkv_host_pallas"])
    if os.path.exists(HOST_PALLAS_API_LIB) and _host_stale(HOST_PALLAS_PROVE_LIB, HOST_PALLAS_API_LIB):
        _gxx(HOST_PALLAS_PROVE_LIB, "capi_pallas_prove.cpp", pasta, "snarkv_pallas", ["snarkv_host_pallas"])
    if os.path.exists(HOST_PALLAS_API_LIB) and _host_stale(HOST_PALLAS_PLONK_PROVE_LIB, HOST_PALLAS_API_LIB):
        _gxx(HOST_PALLAS_PLONK_PROVE_LIB, "capi_pallas_plonk_prove.cpp", pasta, "snarkv_pallas", ["snarkv_host_pallas"])
    if os.path.exists(HOST_PALLAS_API_LIB) and _host_stale(HOST_PALLAS_PLONK_PROVE_CI_LIB, HOST_PALLAS_API_LIB):
        _gxx(HOST_PALLAS_PLONK_PROVE_CI_LIB, "capi_pallas_plonk_prove_ci.cpp", pasta, "snarkv_pallas", ["snarkv_host_pallas"])
    return HOST_LIB


def build_host_driver_pallas():
    build_host_driver()
    return HOST_PALLAS_LIB


def build_host_api_pallas():
    build_host_driver()
    return HOST_PALLAS_API_LIB


def build_host_api_pallas_fold():
    build_host_driver()
    return HOST_PALLAS_FOLD_LIB


def build_host_api_pallas_prove():
    build_host_driver()
    return HOST_PALLAS_PROVE_LIB


def build_host_api_pallas_plonk_prove():
    build_host_driver()
    return HOST_PALLAS_PLONK_PROVE_LIB


def build_host_api_pallas_plonk_prove_ci():
    build_host_driver()
    return HOST_PALLAS_PLONK_PROVE_CI_LIB


if __name__ == "__main__":
    import time

    t = time.time()
    print(build(verbose="-v" in sys.argv), "built in %.1fs" % (time.time() - t))
