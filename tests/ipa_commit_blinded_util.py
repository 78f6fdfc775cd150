"""What tests/test_gpu_ipa_commit_blinded.py and its child process share: a curve's context, key and oracle, and one call of
`commit_blinded_batch_dev` from and to device memory.  The oracle's blinded commitment is its MSM over the key's first n
points and S, with the blind as the last scalar."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)  # the child process starts outside pytest
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import pallas as PA  # noqa: E402

FILL = 0xAB  # what an output buffer holds before a call


def enc(v):
    return b"".join(int(x).to_bytes(32, "little") for x in v)


class Bn:
    """BN254: the C oracle"""
    name, R, pallas = "bn254", O.R, False

    def __init__(self):
        import snark_verifier_amd as sv

        self.ctx = sv.Context(0)
        self.new_ctx = lambda: sv.Context(0)
        self.dk = lambda gb: sv.IpaDecidingKey(self.ctx, gb)

    def key_bytes(self, seed, n):
        return C.sample_points(seed, n)

    def point(self, scalar):
        return O.g1_to_bytes(O.g1_mul(O.G1_GEN, scalar))

    def msm(self, sb, gb):
        return C.msm_pippenger(sb, gb, 4 if len(sb) < 32 * 256 else 8)

    def neg(self, p64):
        y = int.from_bytes(p64[32:], "little")
        return p64[:32] + ((O.P - y) % O.P).to_bytes(32, "little")


class Pa:
    """pallas: the Python oracle"""
    name, R, pallas = "pallas", PA.R, True

    def __init__(self):
        from snark_verifier_amd import pallas as PL

        self.ctx = PL.PallasContext(0)
        self.new_ctx = lambda: PL.PallasContext(0)
        self.dk = lambda gb: self.ctx.ipa_dk_create(gb)

    def key_bytes(self, seed, n):
        return b"".join(PA.g1_to_bytes(p) for p in PA.sample_points(seed, n))

    def point(self, scalar):
        return PA.g1_to_bytes(PA.g1_mul(PA.G1_GEN, scalar))

    def msm(self, sb, gb):
        n = len(sb) // 32
        sc = [int.from_bytes(sb[32 * i:32 * i + 32], "little") for i in range(n)]
        pts = [PA.g1_from_bytes(gb[64 * i:64 * i + 64]) for i in range(n)]
        live = [(s, p) for s, p in zip(sc, pts) if p is not None and s]
        if not live:
            return bytes(64)
        return PA.g1_to_bytes(PA.g1_msm_pippenger([s for s, _ in live], [p for _, p in live]))

    def neg(self, p64):
        return PA.g1_to_bytes(PA.g1_neg(PA.g1_from_bytes(p64)))


def curve(name):
    return Bn() if name == "bn254" else Pa()


def expected(cv, gb, s64, vec, blind):
    """<vec, G[:n]> + blind * S by the oracle's MSM"""
    return cv.msm(enc(list(vec) + [blind % cv.R]), gb[:64 * len(vec)] + s64)


def run(cv, dk, s64, vecs, blinds, slices=0, ctx=None):
    """one call over len(vecs) vectors of equal length -> the output buffer's bytes after the stream has drained"""
    import torch

    from snark_verifier_amd import ipa_commit_blinded as CB

    ctx = ctx or cv.ctx
    n, m = len(vecs[0]), len(vecs)
    d_in = torch.frombuffer(bytearray(b"".join(enc(v) for v in vecs)), dtype=torch.uint8).cuda()
    d_out = torch.full((64 * m,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        CB.commit_blinded_batch_dev(ctx, dk, s64, d_in, n, m, enc(blinds) if blinds is not None else None, d_out, slices)
    finally:
        ctx.sync()
        run.last_out = bytes(d_out.cpu().numpy())
    return run.last_out
