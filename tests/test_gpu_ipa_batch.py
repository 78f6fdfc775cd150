"""GPU: many scalar vectors against one resident IPA key (include/snarkv_ipa_batch.h; csrc/msm_shared.hip), both curves:
`commit_batch` bit for bit against the oracle MSM -- shapes below, at and across the slice and piece boundaries, forced slice
counts, degenerate keys and vectors -- and `decide_batch` through the window table against the per-accumulator route."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import ipa as I  # noqa: E402
import pallas as PA  # noqa: E402

pytestmark = pytest.mark.gpu


class Bn:
    """BN254: the C oracle"""
    name, R, pallas = "bn254", O.R, False

    def __init__(self):
        import snark_verifier_amd as sv

        self.sv = sv
        self.ctx = sv.Context(0)

    def key_bytes(self, seed, n):
        return C.sample_points(seed, n)

    def dk(self, gb):
        return self.sv.IpaDecidingKey(self.ctx, gb)

    def msm(self, sb, gb):
        return C.msm_pippenger(sb, gb, 4 if len(sb) < 32 * 256 else 8)

    def neg(self, p64):
        y = int.from_bytes(p64[32:], "little")
        return p64[:32] + ((O.P - y) % O.P).to_bytes(32, "little")

    def new_ctx(self):
        return self.sv.Context(0)

    def h_coeffs(self, xi):
        return I.h_coeffs(xi, 1)


class Pa:
    """pallas: the Python oracle"""
    name, R, pallas = "pallas", PA.R, True

    def __init__(self):
        from snark_verifier_amd import pallas as PL

        self.PL = PL
        self.ctx = PL.PallasContext(0)

    def key_bytes(self, seed, n):
        return b"".join(PA.g1_to_bytes(p) for p in PA.sample_points(seed, n))

    def dk(self, gb):
        return self.ctx.ipa_dk_create(gb)

    def msm(self, sb, gb):
        n = len(sb) // 32
        sc = [int.from_bytes(sb[32 * i:32 * i + 32], "little") for i in range(n)]
        pts = [PA.g1_from_bytes(gb[64 * i:64 * i + 64]) for i in range(n)]
        live = [(s, p) for s, p in zip(sc, pts) if p is not None]
        if not live:
            return bytes(64)
        return PA.g1_to_bytes(PA.g1_msm_pippenger([s for s, _ in live], [p for _, p in live]))

    def neg(self, p64):
        return PA.g1_to_bytes(PA.g1_neg(PA.g1_from_bytes(p64)))

    def new_ctx(self):
        return self.PL.PallasContext(0)

    def h_coeffs(self, xi):
        out = [1]
        for x in reversed(xi):  # h(X) = prod_i (1 + xi_{k-1-i} X^(2^i)): pcs/ipa.rs:405-421
            out = out + [c * x % PA.R for c in out]
        return out


@pytest.fixture(scope="module", params=["bn254", "pallas"])
def cv(request):
    c = Bn() if request.param == "bn254" else Pa()
    yield c
    c.ctx.close()


def _enc(v):
    return b"".join(int(x).to_bytes(32, "little") for x in v)


def _check_commit(cv, dk, gb, vecs, n):
    got = cv.ctx.ipa_commit_batch(dk, b"".join(_enc(v) for v in vecs), n)
    assert len(got) == 64 * len(vecs)
    for a, v in enumerate(vecs):
        assert got[64 * a:64 * a + 64] == cv.msm(_enc(v), gb[:64 * n]), (cv.name, n, a)
    return got


def test_commit_batch_1024_terms_on_bn254():
    """(10, 1 024, 9): eight slices of 128 terms per vector, the largest slice there is (the C oracle only: the Python
    oracle of pallas is too slow for it)"""
    bn = Bn()
    try:
        test_commit_batch_equals_the_oracle(bn, 10, 1024, 9)
    finally:
        bn.ctx.close()


@pytest.mark.parametrize("k,n,m", [(1, 2, 1), (1, 1, 3), (3, 8, 5), (6, 64, 65), (6, 37, 2)])
def test_commit_batch_equals_the_oracle(cv, k, n, m):
    rnd = random.Random("cb-%d-%d-%d" % (k, n, m))
    gb = cv.key_bytes(300 + k, 1 << k)
    dk = cv.dk(gb)
    assert dk.table_bytes == 0
    _check_commit(cv, dk, gb, [[rnd.randrange(cv.R) for _ in range(n)] for _ in range(m)], n)
    assert dk.table_bytes == 32 * (1 << k) * 64  # built by the first batched call
    dk.close()


@pytest.mark.parametrize("slices", [1, 2, 7])
def test_commit_batch_dev_forced_slices(cv, slices):
    """(6, 64, 3) cut into 1, 2 and 7 slices: the stitching across slices and pieces where a slice holds fewer entries
    than lanes (7 slices of <= 10 terms) and more (1 slice of 64 terms = 2 048 digits)"""
    import torch

    rnd = random.Random("slices")
    n, m = 64, 3
    gb = cv.key_bytes(306, n)
    dk = cv.dk(gb)
    vecs = [[rnd.randrange(cv.R) for _ in range(n)] for _ in range(m)]
    d_in = torch.frombuffer(bytearray(b"".join(_enc(v) for v in vecs)), dtype=torch.uint8).cuda()
    d_out = torch.zeros(64 * m, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cv.ctx.ipa_commit_batch_dev(dk, d_in.data_ptr(), n, m, d_out.data_ptr(), slices)
    cv.ctx.sync()
    got = bytes(d_out.cpu().numpy())
    for a, v in enumerate(vecs):
        assert got[64 * a:64 * a + 64] == cv.msm(_enc(v), gb), (slices, a)
    dk.close()


def test_commit_batch_degenerate_keys_and_vectors(cv):
    rnd = random.Random("degenerate")
    n = 64
    g = cv.key_bytes(77, n)
    pt = lambda i: g[64 * i:64 * i + 64]  # noqa: E731
    put = lambda gb, i, p: gb[:64 * i] + p + gb[64 * i + 64:]  # noqa: E731
    keys = [put(g, 9, pt(3)),            # G[3] == G[9]
            put(g, 6, cv.neg(pt(5))),    # G[5] == -G[6]
            put(g, 11, bytes(64))]       # an identity row
    one_scalar = rnd.randrange(cv.R)
    single = [0] * n
    single[41] = rnd.randrange(1, cv.R)
    vecs = [[0] * n, [1] * n, [cv.R - 1] * n, [one_scalar] * n, single]
    for gb in keys:
        dk = cv.dk(gb)
        got = _check_commit(cv, dk, gb, vecs, n)
        assert got[:64] == bytes(64)  # the all-zero vector: the identity, 64 zero bytes
        dk.close()
    # results that are the identity without a zero scalar: s G[5] + s (-G[5]), and s G + (r - s) G on a doubled base
    dk = cv.dk(keys[1])
    cancel = [0] * n
    cancel[5] = cancel[6] = one_scalar
    assert _check_commit(cv, dk, keys[1], [cancel], n) == bytes(64)
    dk.close()
    dk = cv.dk(keys[0])
    cancel = [0] * n
    cancel[3], cancel[9] = one_scalar, cv.R - one_scalar
    assert _check_commit(cv, dk, keys[0], [cancel], n) == bytes(64)
    dk.close()


def _one_by_one(cv, gb, k, xis, us):
    """the per-accumulator route: one accumulator per call on a fresh key that never gets a table"""
    dk = cv.dk(gb)
    out = []
    for a in range(len(us)):
        out += cv.ctx.ipa_decide_batch(dk, _enc(xis[a]), us[a])
    if os.environ.get("SNARKV_IPA_SHARED") != "1":
        assert dk.table_bytes == 0
    dk.close()
    return out


@pytest.mark.parametrize("k", [3, 8])
def test_decide_batch_through_the_table(cv, k):
    rnd = random.Random("decide-%d" % k)
    n = 1 << k
    gb = cv.key_bytes(500 + k, n)
    m_max = 65
    xis = [[rnd.randrange(cv.R) for _ in range(k)] for _ in range(m_max)]
    helper = cv.dk(gb)  # honest U: the commitments to h_coeffs (commit_batch is checked against the oracle above)
    us_all = cv.ctx.ipa_commit_batch(helper, b"".join(_enc(cv.h_coeffs(x)) for x in xis), n)
    helper.close()
    us = [us_all[64 * a:64 * a + 64] for a in range(m_max)]
    assert us[0] == cv.msm(_enc(cv.h_coeffs(xis[0])), gb)  # ... and the first one here
    other = cv.msm(_enc([1]), gb[:64])
    dk = cv.dk(gb)
    assert dk.table_bytes == 0
    dk.prepare()
    assert dk.table_bytes == 32 * n * 64
    dk.prepare()  # a no-op
    assert dk.table_bytes == 32 * n * 64
    for m in (1, 2, 5, 65):
        assert cv.ctx.ipa_decide_batch(dk, b"".join(_enc(x) for x in xis[:m]), b"".join(us[:m])) == [True] * m
        for pos in sorted({0, m // 2, m - 1}):
            bad_u = list(us[:m])
            bad_u[pos] = other if other != us[pos] else bytes(64)
            bad_x = [list(x) for x in xis[:m]]
            bad_x[pos][k - 1] = (bad_x[pos][k - 1] + 1) % cv.R
            for xs, uu in ((xis[:m], bad_u), (bad_x, us[:m])):
                got = cv.ctx.ipa_decide_batch(dk, b"".join(_enc(x) for x in xs), b"".join(uu))
                assert got == [a != pos for a in range(m)]
                if m <= 5:
                    assert got == _one_by_one(cv, gb, k, xs, uu)
    dk.close()
    # an auto call at or above the threshold builds the table itself
    dk = cv.dk(gb)
    assert cv.ctx.ipa_decide_batch(dk, b"".join(_enc(x) for x in xis), b"".join(us)) == [True] * m_max
    if os.environ.get("SNARKV_IPA_SHARED") != "0":
        assert dk.table_bytes == 32 * n * 64
    dk.close()


def test_flags_and_errors(cv):
    import snark_verifier_amd as sv

    rnd = random.Random("flags")
    n, m = 8, 3
    gb = cv.key_bytes(41, n)
    vecs = [[rnd.randrange(cv.R) for _ in range(n)] for _ in range(m)]
    want = b"".join(cv.msm(_enc(v), gb) for v in vecs)
    ctx = cv.new_ctx()
    dk = cv.dk(gb)
    try:
        for bad in ((b"", n), (b"", 0)):  # m = 0, n = 0
            with pytest.raises(sv.SnarkvError) as e:
                ctx.ipa_commit_batch(dk, *bad)
            assert e.value.code == sv.SNARKV_ERR_EMPTY
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_commit_batch(dk, bytes(32 * (n + 1)), n + 1)  # n > count
        assert e.value.code == sv.SNARKV_ERR_LENGTH
        ctx.set_flags(sv.SNARKV_FLAG_MONTGOMERY)  # the IPA still speaks the wire form
        assert ctx.ipa_commit_batch(dk, b"".join(_enc(v) for v in vecs), n) == want
        ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
        assert ctx.ipa_commit_batch(dk, b"".join(_enc(v) for v in vecs), n) == want
        vecs[m - 1][n - 1] = cv.R  # one non-canonical scalar, the last of the last vector
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_commit_batch(dk, b"".join(_enc(v) for v in vecs), n)
        assert e.value.code == sv.SNARKV_ERR_ENCODING
        ctx.set_flags(0)  # without the flag the value is taken modulo r
        vecs[m - 1][n - 1] = 0
        got = ctx.ipa_commit_batch(dk, b"".join(_enc(v) for v in vecs[:m - 1]) + _enc(vecs[m - 1][:n - 1] + [cv.R]), n)
        assert got[64 * (m - 1):] == cv.msm(_enc(vecs[m - 1]), gb)
    finally:
        dk.close()
        ctx.close()


def test_two_host_threads_share_an_unprepared_key(cv):
    """the context-free forms on one key handle from two threads at once: one table, right verdicts"""
    from snark_verifier_amd import ipa_batch

    rnd = random.Random("threads")
    k, m = 6, 8
    n = 1 << k
    gb = cv.key_bytes(88, n)
    xis = [[rnd.randrange(cv.R) for _ in range(k)] for _ in range(m)]
    us = [cv.msm(_enc(cv.h_coeffs(x)), gb) if a % 3 else bytes(64) for a, x in enumerate(xis)]
    want = [a % 3 != 0 for a in range(m)]
    lib = ipa_batch.api(cv.pallas).lib
    pre = "pallas" if cv.pallas else "bn254"
    create, decide = getattr(lib, pre + "_ipa_dk_create"), getattr(lib, pre + "_ipa_decide_batch")
    vp = ctypes.c_void_p
    create.restype, create.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    decide.restype, decide.argtypes = ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, vp]
    h = vp()
    assert create(gb, n, ctypes.byref(h)) == 0
    xb, ub = b"".join(_enc(x) for x in xis), b"".join(us)
    res = [None, None]
    start = threading.Barrier(2)

    def work(i):
        ok = ctypes.create_string_buffer(m)
        start.wait()
        rc = decide(h, xb, ub, m, ok)
        res[i] = (rc, [b != 0 for b in ok.raw])

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res[0] == (0, want) and res[1] == (0, want)

    class _K:
        _h = h

    if os.environ.get("SNARKV_IPA_SHARED") != "0":
        assert ipa_batch.dk_table_bytes(_K, cv.pallas) == 32 * n * 64
    getattr(lib, ("snarkv_pallas" if cv.pallas else "snarkv") + "_ipa_dk_destroy")(h)


@pytest.fixture(scope="module")
def forged(tmp_path_factory):
    """four PLONK-over-IPA proofs at k = 8, forged once for both settings of the knob"""
    path = str(tmp_path_factory.mktemp("ipa_batch") / "proofs.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ipa_batch_product_child.py"), "--forge", path], check=True,
                   timeout=600)
    return path


@pytest.mark.parametrize("knob", ["1", "0"])
def test_plonk_verify_under_the_override(forged, knob):
    """`host_api_pallas.plonk_verify` (succinct half, then `decide_all`) on PLONK-over-IPA proofs at k = 8, forged as
    tools/bench_pallas_verify.py forges its 64 (the tree holds no committed ones; four keep the pure-Python forging to
    seconds), with SNARKV_IPA_SHARED = 1 and = 0 (read once: a child process each): accepts, and rejects with one
    proof's U replaced."""
    script = os.path.join(ROOT, "tests", "ipa_batch_product_child.py")
    r = subprocess.run([sys.executable, script, forged], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SNARKV_IPA_SHARED=knob))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accept=True reject=True" in r.stdout, r.stdout + r.stderr
