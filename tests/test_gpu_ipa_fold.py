"""GPU: `IpaAs::decide_all` as one folded check (include/snarkv_ipa_fold.h; csrc/ipa_fold.hip), both curves: the fold kernel
against the big-integer definition and, bit for bit, against `snarkv_ipa_as_combine_dev`; the folded decide on valid and
invalid batches, with weights that are really applied, rejects that are not errors, the error codes, and a key with and
without its window table; the product API of the pallas host mirror in a child process."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import pallas as PA  # noqa: E402
from test_ipa_fold_model import fold_definition  # noqa: E402

pytestmark = pytest.mark.gpu


def _enc(v):
    return b"".join(int(x).to_bytes(32, "little") for x in v)


def _h_coeffs(xi, r):
    out = [1]
    for x in reversed(xi):  # h(X) = prod_i (1 + xi_{k-1-i} X^(2^i)): pcs/ipa.rs:405-421
        out = out + [c * x % r for c in out]
    return out


class Bn:
    """BN254: the C oracle"""
    name, R, P, pallas = "bn254", O.R, O.P, False

    def __init__(self):
        import snark_verifier_amd as sv

        self.sv = sv
        self.ctx = sv.Context(0)

    def new_ctx(self):
        return self.sv.Context(0)

    def key_bytes(self, seed, n):
        return C.sample_points(seed, n)

    def dk(self, gb, ctx=None):
        return self.sv.IpaDecidingKey(ctx or self.ctx, gb)

    def shard(self, gb, k, first):
        return self.sv.IpaDecidingKey(self.ctx, gb, k=k, first=first)

    def msm(self, sb, gb):
        return C.msm_pippenger(sb, gb, 4 if len(sb) < 32 * 256 else 8)

    def add(self, p64, q64):
        return C.g1_add(p64, q64)

    def neg(self, p64):
        y = int.from_bytes(p64[32:], "little")
        return p64[:32] + ((O.P - y) % O.P).to_bytes(32, "little")


class Pa:
    """pallas: the Python oracle"""
    name, R, P, pallas = "pallas", PA.R, PA.P, True

    def __init__(self):
        from snark_verifier_amd import pallas as PL

        self.PL = PL
        self.ctx = PL.PallasContext(0)

    def new_ctx(self):
        return self.PL.PallasContext(0)

    def key_bytes(self, seed, n):
        return b"".join(PA.g1_to_bytes(p) for p in PA.sample_points(seed, n))

    def dk(self, gb, ctx=None):
        return (ctx or self.ctx).ipa_dk_create(gb)

    def shard(self, gb, k, first):
        h = ctypes.c_void_p()
        lib = self.ctx._lib
        assert lib.snarkv_pallas_ipa_dk_create_shard(self.ctx._h, gb, len(gb) // 64, k, first, ctypes.byref(h)) == 0
        return self.PL.PallasIpaDecidingKey(lib, h, self.ctx)

    def msm(self, sb, gb):
        n = len(sb) // 32
        sc = [int.from_bytes(sb[32 * i:32 * i + 32], "little") for i in range(n)]
        pts = [PA.g1_from_bytes(gb[64 * i:64 * i + 64]) for i in range(n)]
        return PA.g1_to_bytes(PA.g1_msm_pippenger(sc, pts))

    def add(self, p64, q64):
        return PA.g1_to_bytes(PA.g1_add(PA.g1_from_bytes(p64), PA.g1_from_bytes(q64)))

    def neg(self, p64):
        return PA.g1_to_bytes(PA.g1_neg(PA.g1_from_bytes(p64)))


@pytest.fixture(scope="module", params=["bn254", "pallas"])
def cv(request):
    c = Bn() if request.param == "bn254" else Pa()
    c.batches = {}
    yield c
    c.ctx.close()


def _batch(cv, k, m=5):
    """m valid accumulators over a key of 2^k points, U = msm(h_coeffs(xi), G) from the oracle: computed once per curve"""
    if (k, m) not in cv.batches:
        rnd = random.Random("fold-batch-%s-%d-%d" % (cv.name, k, m))
        gb = cv.key_bytes(700 + k, 1 << k)
        xis = [[rnd.randrange(cv.R) for _ in range(k)] for _ in range(m)]
        us = [cv.msm(_enc(_h_coeffs(x, cv.R)), gb) for x in xis]
        cv.batches[(k, m)] = (gb, xis, us)
    gb, xis, us = cv.batches[(k, m)]
    return gb, [list(x) for x in xis], list(us)


def _xb(xis):
    return b"".join(_enc(x) for x in xis)


# (k, m, slices): a key smaller than a lane's block of 8 coefficients, exactly one block, more than one workgroup of blocks,
# a ragged last slice, more slices than accumulators per slice; the last three pass through the reduction of the lazy sums
# after 32 additions (in a slice, and over the slices) and the power table through more than one workgroup
SHAPES = [(1, 1, 0), (1, 3, 1), (2, 5, 2), (3, 8, 7), (4, 65, 0), (9, 9, 2), (9, 65, 7), (5, 70, 1), (3, 70, 35), (1, 4100, 0),
          (1, 40000, 40000)]  # ... and more slices asked for than the launch takes (32 768)


@pytest.mark.parametrize("k,m,slices", SHAPES)
def test_fold_coeffs_equal_the_definition_and_as_combine(cv, k, m, slices):
    import torch

    from snark_verifier_amd import ipa_prover

    rnd = random.Random("fold-coeffs-%d-%d-%d" % (k, m, slices))
    n = 1 << k
    xis = [[rnd.randrange(cv.R) for _ in range(k)] for _ in range(m)]
    d_h = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    d_ref = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for rho in (rnd.randrange(cv.R), 0, 1, cv.R - 1):
        d_h.fill_(0xA5)
        torch.cuda.synchronize()
        cv.ctx.ipa_fold_coeffs_dev(k, _xb(xis), rho, d_h.data_ptr(), slices)
        cv.ctx.sync()
        got = bytes(d_h.cpu().numpy())
        assert got == _enc(fold_definition(xis, rho, cv.R)), (cv.name, k, m, slices, rho)
        ipa_prover.as_combine_dev(cv.ctx, xis, rho, None, d_ref.data_ptr())
        cv.ctx.sync()
        assert got == bytes(d_ref.cpu().numpy()), (cv.name, k, m, slices, rho)


@pytest.mark.parametrize("k", [3, 8])
def test_decide_folded_accepts_valid_and_rejects_a_negated_u(cv, k):
    gb, xis, us = _batch(cv, k)
    m = len(us)
    rho = random.Random("rho-%d" % k).randrange(cv.R)
    dk = cv.dk(gb)
    try:
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), rho) is True
        for pos in (0, m // 2, m - 1):
            bad = list(us)
            bad[pos] = cv.neg(us[pos])
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(bad), rho) is False, pos
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis[:1]), us[0], rho) is True
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis[:1]), us[1], rho) is False
        # on the library's default context, with a rho derived from the batch
        from snark_verifier_amd import ipa_fold

        rho = ipa_fold.fold_challenge(k, _xb(xis), b"".join(us), cv.pallas)

        assert ipa_fold.decide_folded_default(dk, _xb(xis), b"".join(us), rho, cv.pallas) is True
        assert ipa_fold.decide_folded_default(dk, _xb(xis), b"".join(us[1:] + us[:1]), rho, cv.pallas) is False
    finally:
        dk.close()


def test_the_weights_are_applied(cv):
    """U_a + D and U_b - D cancel under equal weights only: rho = 1 accepts, rho = 2 rejects"""
    k = 3
    gb, xis, us = _batch(cv, k)
    d = gb[64:128]  # a point of the curve
    us[1] = cv.add(us[1], d)
    us[3] = cv.add(us[3], cv.neg(d))
    dk = cv.dk(gb)
    try:
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), 1) is True
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), 2) is False
    finally:
        dk.close()


def test_bad_points_are_rejects_not_errors(cv):
    k = 3
    gb, xis, us = _batch(cv, k)
    rho = 0x1234567 % cv.R
    dk = cv.dk(gb)
    try:
        x, y = int.from_bytes(us[2][:32], "little"), int.from_bytes(us[2][32:], "little")
        off_curve = us[2][:32] + ((y + 1) % cv.P).to_bytes(32, "little")
        too_big = (x + cv.P).to_bytes(32, "little") + us[2][32:]  # x + p < 2^256 on both curves
        for bad in (off_curve, too_big, bytes(64)):
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis[2:3]), bad, rho) is False
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us[:2] + [bad] + us[3:]), rho) is False
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), rho) is True
    finally:
        dk.close()


def test_errors_leave_the_context_usable(cv):
    import snark_verifier_amd as sv

    k = 3
    gb, xis, us = _batch(cv, k)
    rho = 77
    ctx = cv.new_ctx()
    dk = cv.dk(gb)
    shard = cv.shard(gb[:64 * 4], k, 0)
    try:
        def good():
            return ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), rho)

        assert good() is True  # the key of another context on the same device serves
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_decide_folded(shard, _xb(xis), b"".join(us), rho)
        assert e.value.code == sv.SNARKV_ERR_LENGTH
        assert good() is True
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_decide_folded(dk, b"", b"", rho)
        assert e.value.code == sv.SNARKV_ERR_EMPTY
        assert good() is True
        ctx.set_flags(sv.SNARKV_FLAG_VALIDATE)
        assert good() is True
        bad_x = [list(x) for x in xis]
        bad_x[-1][-1] = cv.R  # the last challenge of the last accumulator
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_decide_folded(dk, _xb(bad_x), b"".join(us), rho)
        assert e.value.code == sv.SNARKV_ERR_ENCODING
        assert good() is True
        with pytest.raises(sv.SnarkvError) as e:
            ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), cv.R)
        assert e.value.code == sv.SNARKV_ERR_ENCODING
        assert good() is True
        ctx.set_flags(0)  # without the flag the values are taken modulo r
        bad_x[-1][-1] = xis[-1][-1] + cv.R  # below 2^256 on both curves
        assert ctx.ipa_decide_folded(dk, _xb(bad_x), b"".join(us), rho) is True
    finally:
        shard.close()
        dk.close()
        ctx.close()


@pytest.mark.parametrize("k", [3, 8])
def test_a_key_with_and_without_its_table_give_the_same_verdicts(cv, k):
    gb, xis, us = _batch(cv, k)
    rho = random.Random("table-%d" % k).randrange(cv.R)
    with_table, without = cv.dk(gb), cv.dk(gb)
    try:
        with_table.prepare()
        assert with_table.table_bytes == 32 * (1 << k) * 64 and without.table_bytes == 0
        swapped = us[1:] + us[:1]
        for dk in (with_table, without):
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(us), rho) is True
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis), b"".join(swapped), rho) is False
            assert cv.ctx.ipa_decide_folded(dk, _xb(xis[:1]), us[0], rho) is True
        assert without.table_bytes == 0  # the folded decide never builds the table
    finally:
        with_table.close()
        without.close()


@pytest.mark.parametrize("k,m", [(13, 3), (1, 4100)])
def test_the_msms_above_the_naive_threshold(cv, k, m):
    """more than 4 096 terms take the Pippenger: the 2^k-term MSM at k = 13, the m-term one at m = 4 100.  The honest U
    come from `ipa_commit_batch` over h_coeffs (checked against the oracle in tests/test_gpu_ipa_batch.py) and are
    confirmed by the per-accumulator `ipa_decide_batch`; the key repeats 64 sampled points, which a committing key may."""
    rnd = random.Random("fold-pip-%d-%d" % (k, m))
    n = 1 << k
    base = cv.key_bytes(900 + k, min(n, 64))
    gb = base * (n // min(n, 64))
    xis = [[rnd.randrange(cv.R) for _ in range(k)] for _ in range(m)]
    helper, dk = cv.dk(gb), cv.dk(gb)
    try:
        us_all = cv.ctx.ipa_commit_batch(helper, b"".join(_enc(_h_coeffs(x, cv.R)) for x in xis), n)
        assert cv.ctx.ipa_decide_batch(helper, _xb(xis), us_all) == [True] * m
        rho = rnd.randrange(cv.R)
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis), us_all, rho) is True
        swapped = us_all[:64 * (m - 2)] + us_all[64 * (m - 1):] + us_all[64 * (m - 2):64 * (m - 1)]
        assert swapped != us_all
        assert cv.ctx.ipa_decide_folded(dk, _xb(xis), swapped, rho) is False
        assert dk.table_bytes == 0
    finally:
        helper.close()
        dk.close()


def test_product_api_of_the_pallas_host_mirror(tmp_path):
    """`host_api_pallas.ipa_decide_all_folded` / `plonk_verify_folded` (include/snarkv_host_pallas_fold.h) on forged
    PLONK-over-IPA proofs at k = 8, in a child process as tests/ipa_batch_product_child.py runs its own"""
    script = os.path.join(ROOT, "tests", "ipa_fold_product_child.py")
    path = str(tmp_path / "proofs.json")
    subprocess.run([sys.executable, script, "--forge", path], check=True, timeout=600)
    r = subprocess.run([sys.executable, script, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "folded_accept=True folded_reject=True culprit=True plonk_equal=True" in r.stdout, r.stdout + r.stderr
