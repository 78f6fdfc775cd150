"""GPU parity of the Pippenger piece schedule: a bucket of cnt entries is cut into ceil(cnt / L) pieces of at most L
entries (L = 16 / 32 for one small MSM, 128 under the throughput hint), one k_accumulate lane per piece, and k_fixup
stitches split buckets and redoes degenerate ones.  Every case compares affine bytes with the C oracle, or with the
unsplit single call where the oracle would be too slow."""
import pytest

import bn254 as O
import coracle as C

pytestmark = pytest.mark.gpu

# The caps under test: 32 = one MSM of a few thousand points without the hint (latency_run_length), 128 = the hint.
CAPS = (32, 128)


def _dev(b):
    import torch

    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _run(ctx, s, p, c=0):
    import torch

    ds, dp = _dev(s), _dev(p)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.msm_pippenger_dev(ds.data_ptr(), dp.data_ptr(), len(s) // 32, out.data_ptr(), window_bits=c)
    ctx.sync()
    return bytes(out.cpu().numpy())


def _both_modes(s, p, c=0):
    """bytes of the call without and with the throughput hint (two caps), which must agree with the oracle"""
    import snark_verifier_amd as sv

    exp = C.msm_pippenger(s, p, 4)
    for hint in (False, True):
        ctx = sv.Context(0)
        ctx.set_throughput_hint(hint)
        try:
            assert _run(ctx, s, p, c) == exp, ("hint" if hint else "no hint", c)
        finally:
            ctx.close()


def _small_scalar_buckets(lengths, n_fill, seed):
    """Scalars d < 2^15 (GLV halves (d, 0): one digit, window 0 only at c = 16) so that bucket d - 1 of window 0 gets
    exactly the requested number of entries; `n_fill` more scalars spread one per bucket above them.  Every other
    window's buckets are empty."""
    sc = []
    for i, ln in enumerate(lengths):
        sc += [2 * i + 3] * ln
    sc += [1000 + 7 * i for i in range(n_fill)]
    n = len(sc)
    return b"".join(O.fe_to_bytes(x) for x in sc), C.sample_points(seed, n)


def test_bucket_lengths_around_the_cap():
    lengths = []
    for L in CAPS:
        lengths += [L - 1, L, L + 1, 2 * L + 1]
    s, p = _small_scalar_buckets(lengths, 300, 0xB1)
    _both_modes(s, p, c=16)


def test_all_scalars_equal_and_half_equal():
    n = 1 << 14
    p = C.sample_points(0xB2, n)
    k = O.fe_from_bytes(C.sample_scalars(0xB3, 1))
    s = O.fe_to_bytes(k) * n
    _both_modes(s, p)
    half = bytearray(C.sample_scalars(0xB4, n))
    half[: 32 * (n // 2)] = O.fe_to_bytes(k) * (n // 2)
    _both_modes(bytes(half), p)


def test_zero_scalars_and_empty_buckets():
    n = 600
    s = bytearray(C.sample_scalars(0xB5, n))
    for i in range(0, n, 3):
        s[32 * i:32 * i + 32] = bytes(32)
    p = C.sample_points(0xB6, n)
    _both_modes(bytes(s), p, c=17)  # 2^16 buckets per window for 800 non-zero scalars: almost all empty
    _both_modes(bytes(32) * n, p)   # every scalar zero: the identity


def _with_points(lengths, plan, seed):
    """buckets of the given lengths (as _small_scalar_buckets); plan[i] = list of (j, kind): entry j of bucket i becomes
    a copy ('dup') or the negation ('neg') of entry 0 of that bucket"""
    s, p = _small_scalar_buckets(lengths, 50, seed)
    p = bytearray(p)
    starts = [sum(lengths[:i]) for i in range(len(lengths))]
    for i, marks in plan.items():
        base = O.g1_from_bytes(bytes(p[64 * starts[i]:64 * starts[i] + 64]))
        for j, kind in marks:
            q = base if kind == "dup" else O.g1_neg(base)
            p[64 * (starts[i] + j):64 * (starts[i] + j + 1)] = O.g1_to_bytes(q)
    return s, bytes(p)


@pytest.mark.parametrize("kind", ["dup", "neg"])
def test_duplicate_and_opposite_points(kind):
    """P twice / P and -P in one bucket: in a whole bucket (one piece), in a split bucket (the two entries land in one
    piece or in two, depending on where the sort puts them), and in every entry of a bucket of 2L + 1"""
    lengths = [5, 20, 33, 40, 129, 200, 65, 257]
    plan = {0: [(1, kind)], 1: [(19, kind)], 2: [(32, kind)], 3: [(1, kind), (39, kind)], 4: [(128, kind)],
            5: [(100, kind)]}
    plan[6] = [(j, kind if j % 2 else "dup") for j in range(1, 65)]   # P, -P / P, P ... across the pieces
    plan[7] = [(j, "dup") for j in range(1, 257)]                      # one point 257 times
    s, p = _with_points(lengths, plan, 0xB7 if kind == "dup" else 0xB8)
    _both_modes(s, p, c=16)


@pytest.mark.parametrize("c", [13, 14, 15, 16, 17])
def test_window_sizes_13_to_17(c):
    n = 3000
    _both_modes(C.sample_scalars(0xC0 + c, n), C.sample_points(0xD0 + c, n), c=c)


def test_batch_of_mixed_sizes(gpu_ctx):
    import torch

    sizes = [1, 4097, 70000, 3, (1 << 16) + 3]
    ss = [C.sample_scalars(0xE0 + i, n) for i, n in enumerate(sizes)]
    ps = [C.sample_points(0xE8 + i, n) for i, n in enumerate(sizes)]
    # one job of all-equal scalars: its buckets split into many pieces next to jobs that do not
    ss[3] = O.fe_to_bytes(12345) * sizes[3]
    ss.append(O.fe_to_bytes(O.R - 99) * 5000)
    ps.append(C.sample_points(0xEF, 5000))
    sizes.append(5000)
    ds, dp = [_dev(x) for x in ss], [_dev(x) for x in ps]
    out = torch.zeros(64 * len(sizes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.msm_pippenger_many_dev([t.data_ptr() for t in ds], [t.data_ptr() for t in dp], sizes, out.data_ptr())
    gpu_ctx.sync()
    got = bytes(out.cpu().numpy())
    for i in range(len(sizes)):
        assert got[64 * i:64 * i + 64] == C.msm_pippenger(ss[i], ps[i], 4), i


def test_chunk_pipeline_equals_single_launch(gpu_ctx, monkeypatch):
    """3 * 2^20 points: the chunk pipeline (private lanes under the hint's cap) and the single launch (one MSM's cap)
    give the same bytes, for uniform scalars and for scalars that are all equal in one chunk"""
    import torch

    n = 3 << 20
    ds = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    dp = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.sample_scalars_dev(0xF1, n, ds.data_ptr())
    gpu_ctx.sample_points_dev(0xF2, n, dp.data_ptr())
    gpu_ctx.sync()
    for skew in (False, True):
        if skew:
            ds[32 * (1 << 20):32 * (2 << 20)] = ds[:32].repeat(1 << 20)
            torch.cuda.synchronize()
        for k, split in enumerate(("1", "0")):
            monkeypatch.setenv("SNARKV_PIP_SPLIT", split)
            gpu_ctx.msm_pippenger_dev(ds.data_ptr(), dp.data_ptr(), n, out[k].data_ptr())
            gpu_ctx.sync()
        a = bytes(out[0].cpu().numpy())
        assert a == bytes(out[1].cpu().numpy()) and a != bytes(64), skew
    del ds, dp
    torch.cuda.empty_cache()


@pytest.mark.parametrize("hint", [False, True])
def test_bucket_sharded_grids_with_split_buckets(hint):
    """emulated ranks fill the global bucket grid from their shards (skewed: one scalar repeated, so buckets split into
    many pieces) and add the grids: the reduce of the sum equals the unsplit single call"""
    import torch

    import snark_verifier_amd as sv
    from snark_verifier_amd.distributed import shard_range

    n, world = 20000, 3
    s = bytearray(C.sample_scalars(0xF3, n))
    s[: 32 * (n // 2)] = s[:32] * (n // 2)
    s = bytes(s)
    p = C.sample_points(0xF4, n)
    ctx = sv.Context(0)
    ctx.set_throughput_hint(hint)
    try:
        c, W, B = sv.Context.bucket_geometry(n)
        ds, dp = _dev(s), _dev(p)
        PB = sv.G1_PARTIAL_BYTES
        grids = torch.zeros(world, W * B * PB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for r in range(world):
            lo, hi = shard_range(n, r, world)
            ctx.fill_buckets_dev(ds.data_ptr() + 32 * lo, dp.data_ptr() + 64 * lo, hi - lo, c, grids[r].data_ptr())
        for r in range(1, world):
            ctx.buckets_add_dev(grids[0].data_ptr(), grids[r].data_ptr(), W * B)
        part = torch.zeros(PB, dtype=torch.uint8, device="cuda")
        ctx.buckets_reduce_dev(grids[0].data_ptr(), c, 0, W, part.data_ptr())
        out = torch.zeros(64, dtype=torch.uint8, device="cuda")
        ctx.fold_partials_dev(part.data_ptr(), 1, out.data_ptr())
        ctx.sync()
        assert bytes(out.cpu().numpy()) == _run(ctx, s, p, c)
    finally:
        ctx.close()
