"""GPU: the whole decide through the product API on many deciding keys and accumulators, against the C oracle
(coracle.kzg_pairing_value / kzg_decide / kzg_decide_all -- independent of the kernels).  tests/golden/kzg_decider.json
gives k_g2_prepare_w one key and the kernels eight accumulators; here six keys (related, unrelated, s_g2 == g2, a point at
the identity) are each loaded in the wire form and in the in-memory form, 64 accumulators per key cover the identity,
lhs == +-rhs and G1 coordinates next to the 29-bit limb boundaries, and mixed accept / reject batches straddle the
m <= 256 switch of launch_decide with the verdicts at known positions."""
import random

import pytest

import bn254 as O
import coracle as C
import mont_util as MU

pytestmark = pytest.mark.gpu

FORMS = ["1", "3"]


def _sv():
    import snark_verifier_amd as sv

    return sv


def _g1_at(x, step):
    """the first curve point whose x is reached from `x` in steps of `step` (p = 3 mod 4: one power gives the root)"""
    while True:
        rhs = (x * x * x + O.B1) % O.P
        y = pow(rhs, (O.P + 1) // 4, O.P)
        if y * y % O.P == rhs:
            return x, y
        x += step


def _edge_points():
    """G1 points (cofactor 1: every curve point is in the group) with x at the ends of [1, p) and on both sides of every
    2^(29 k) -- the limb boundaries fq29_from_words splits at --, both signs of y: 36 points"""
    xs = [_g1_at(1, 1), _g1_at(O.P - 1, -1)]
    for k in range(1, 9):
        xs += [_g1_at(1 << (29 * k), 1), _g1_at((1 << (29 * k)) - 1, -1)]
    pts = []
    for x, y in xs:
        assert O.g1_is_on_curve((x, y))
        pts += [O.g1_to_bytes((x, y)), O.g1_to_bytes((x, O.P - y))]
    return pts


def _keys(golden):
    """(name, g2, s_g2, s or None): s_g2 = s * g2 where the test knows s"""
    rnd = random.Random(0xD0C1DE)
    big = lambda: rnd.randrange(1, O.R)  # noqa: E731
    a, s, b, c, d, e = (big() for _ in range(6))
    g2a, g2d = O.g2_mul(O.G2_GEN, a), O.g2_mul(O.G2_GEN, d)
    return [
        ("golden", bytes.fromhex(golden["g2"]), bytes.fromhex(golden["s_g2"]), int(golden["secret"], 16)),
        ("related", O.g2_to_bytes(g2a), O.g2_to_bytes(O.g2_mul(g2a, s)), s),
        ("unrelated", O.g2_to_bytes(O.g2_mul(O.G2_GEN, b)), O.g2_to_bytes(O.g2_mul(O.G2_GEN, c)), None),
        ("s_g2_is_g2", O.g2_to_bytes(g2d), O.g2_to_bytes(g2d), 1),
        ("s_g2_identity", O.g2_to_bytes(O.G2_GEN), O.g2_to_bytes(None), 0),
        ("g2_identity", O.g2_to_bytes(None), O.g2_to_bytes(O.g2_mul(O.G2_GEN, e)), None),
    ]


KEY_NAMES = ["golden", "related", "unrelated", "s_g2_is_g2", "s_g2_identity", "g2_identity"]


def _neg(pt):
    return O.g1_to_bytes(O.g1_neg(O.g1_from_bytes(pt)))


def _accumulators(idx, s, edges):
    """64 accumulators (lhs | rhs) for key number idx"""
    pts = C.sample_points(0xACC0 + idx, 64)
    pt = lambda i: pts[64 * i:64 * i + 64]  # noqa: E731
    zero = bytes(64)
    sk = O.fe_to_bytes((s if s is not None else 0x5EC) % O.R)
    accs = [pt(2 * i) + pt(2 * i + 1) for i in range(12)]                      # random pairs
    accs += [C.g1_mul(pt(24 + i), sk) + pt(24 + i) for i in range(8)]          # (s R, R): accepted where s is the key's
    accs += [zero + pt(32), pt(33) + zero, zero + zero]                        # the identity on either side and on both
    accs += [pt(34) + pt(34), pt(35) + pt(35)]                                 # lhs == rhs
    accs += [pt(36) + _neg(pt(36)), pt(37) + _neg(pt(37))]                     # rhs == -lhs
    for i, e in enumerate(edges):                                              # edge coordinates, on either side
        accs.append(e + pt(38 + i % 20) if i % 2 == 0 else pt(38 + i % 20) + e)
    accs.append(edges[0] + edges[-1])
    assert len(accs) == 64
    return accs


@pytest.fixture(scope="module")
def material(golden_decider):
    """per key: its points, its 64 accumulators and the oracle's Gt bytes and verdicts -- computed once for both forms"""
    edges = _edge_points()
    assert len(edges) == 36
    out = {}
    for idx, (name, g2, s_g2, s) in enumerate(_keys(golden_decider)):
        accs = _accumulators(idx, s, edges)
        gts = [C.kzg_pairing_value(g2, s_g2, a) for a in accs]
        oks = [C.kzg_decide(g2, s_g2, a) for a in accs]
        allok, each = C.kzg_decide_all(g2, s_g2, b"".join(accs), threads=4)
        assert each == oks and allok == all(oks)
        if s is not None and s != 0:
            assert all(oks[12:20]), name  # the test has accepting accumulators where it knows the secret
        assert not all(oks) and oks[22], name  # ... rejecting ones everywhere; (identity, identity) is accepted by any key
        out[name] = (g2, s_g2, accs, gts, oks, s)
    assert list(out) == KEY_NAMES
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", KEY_NAMES)
def test_gt_value_and_verdict_per_key(gpu_ctx, material, key, form, monkeypatch):
    """every key loaded in the wire form and in the in-memory form (validated): the exact Gt element and the verdict of
    each of its 64 accumulators, a quarter of them passed in the in-memory form as well"""
    sv = _sv()
    monkeypatch.setenv("SNARKV_DECIDE_FORM", form)
    g2, s_g2, accs, gts, oks, _ = material[key]
    g1 = O.g1_to_bytes(O.G1_GEN)
    FM = sv.SNARKV_FLAG_MONTGOMERY
    dkc = sv.DecidingKey(gpu_ctx, g1, g2, s_g2)
    dkm = sv.DecidingKey(gpu_ctx, MU.coords_to_mont(g1), MU.coords_to_mont(g2), MU.coords_to_mont(s_g2), FM | sv.SNARKV_FLAG_VALIDATE)
    try:
        for i, acc in enumerate(accs):
            for dk in (dkc, dkm):
                assert gpu_ctx.pairing_value(dk, acc) == gts[i], (key, i)
                assert gpu_ctx.decide(dk, acc) == oks[i], (key, i)
            if i % 4 == 0:
                assert gpu_ctx.decide(dkm, MU.coords_to_mont(acc), FM) == oks[i], (key, i)
                assert gpu_ctx.decide(dkc, MU.coords_to_mont(acc), FM | sv.SNARKV_FLAG_VALIDATE) == oks[i], (key, i)
        for dk in (dkc, dkm):
            assert gpu_ctx.decide_batch(dk, b"".join(accs)) == (all(oks), oks), key
    finally:
        dkc.close(), dkm.close()


# ---- mixed batches on both sides of launch_decide's m <= 256 switch -------------------------------------------------
BATCH_SIZES = [255, 256, 257, 300]
_batches = {}


def _accepts(i, m):
    """accepting positions: the first, the last and every fifth from 2 -- so that 1 and m - 2 reject at every size used
    and a verdict written to a neighbouring index shows"""
    return i == 0 or i == m - 1 or i % 5 == 2


def _mixed_batch(material, m):
    if m not in _batches:
        g2, s_g2, accs, _, _, s = material["related"]
        sk, sk1 = O.fe_to_bytes(s), O.fe_to_bytes((s + 1) % O.R)
        pts = C.sample_points(0xBA7C4, m)
        batch = []
        for i in range(m):
            r = pts[64 * i:64 * i + 64]
            if _accepts(i, m):
                batch.append(C.g1_mul(r, sk) + r)
            elif i % 3 == 0:
                batch.append(C.g1_mul(r, sk1) + r)  # one off the secret
            elif i % 3 == 1:
                batch.append(accs[i % 12][:64] + r)  # unrelated points
            else:
                batch.append(r + C.g1_mul(r, sk))  # the sides exchanged
        blob = b"".join(batch)
        allok, oks = C.kzg_decide_all(g2, s_g2, blob, threads=8)
        assert oks == [_accepts(i, m) for i in range(m)] and not allok
        assert not _accepts(1, m) and not _accepts(m - 2, m)
        _batches[m] = (blob, oks)
    return _batches[m]


@pytest.fixture(scope="module")
def related_dk(gpu_ctx, material):
    g2, s_g2 = material["related"][:2]
    dk = _sv().DecidingKey(gpu_ctx, O.g1_to_bytes(O.G1_GEN), g2, s_g2, flags=_sv().SNARKV_FLAG_VALIDATE)
    yield dk
    dk.close()


@pytest.mark.parametrize("form", [None] + FORMS)
@pytest.mark.parametrize("m", BATCH_SIZES)
def test_mixed_batch_verdicts_by_position(gpu_ctx, material, related_dk, m, form, monkeypatch):
    if form is None:
        monkeypatch.delenv("SNARKV_DECIDE_FORM", raising=False)
    else:
        monkeypatch.setenv("SNARKV_DECIDE_FORM", form)
    blob, oks = _mixed_batch(material, m)
    allok, got = gpu_ctx.decide_batch(related_dk, blob)
    assert got == oks, [i for i in range(m) if got[i] != oks[i]]
    assert allok is False


def test_mixed_batch_device_resident(gpu_ctx, material, related_dk, monkeypatch):
    """decide_batch_dev just past the switch: accumulators and verdict bytes stay on the device"""
    import torch

    monkeypatch.delenv("SNARKV_DECIDE_FORM", raising=False)
    m = 257
    blob, oks = _mixed_batch(material, m)
    d_accs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_ok = torch.full((m + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.decide_batch_dev(related_dk, d_accs.data_ptr(), m, d_ok.data_ptr())
    gpu_ctx.sync()
    raw = bytes(d_ok.cpu().numpy())
    assert [b != 0 for b in raw[:m]] == oks and set(raw[:m]) <= {0, 1}
    assert raw[m:] == b"\xEE" * 64  # nothing written past the batch
