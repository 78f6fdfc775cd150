"""GPU parity of the Pippenger piece schedule: a bucket of cnt entries is cut into ceil(cnt / L) pieces of at most L
entries (L = 16 / 32 for one small MSM, 128 under the throughput hint), one k_accumulate lane per piece, and k_fixup
stitches split buckets and redoes degenerate ones.  Every case compares affine bytes with the C oracle, or with the
unsplit single call where the oracle would be too slow.  The second half plans its buckets (tests/msm_edge_util.py) to
reach the fix-up's redo paths, the cap 16, the level-2 sort at its LDS cap, carry chains of the recoders and the tiles."""
import pytest

import bn254 as O
import coracle as C
import msm_edge_util as E

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


# ---- planned buckets at the schedule's edges (tests/msm_edge_util.py; the inputs are checked in tests/test_msm_edge_util.py) ----
BN = E.curve("bn254")
FILL = [1000 + 7 * i for i in range(300)]  # about 300 ordinary buckets next to the planned ones


def test_geometry_restated_in_the_helper_matches_the_library():
    import snark_verifier_amd as sv

    for n in (1, 300, 2000, 7168, 1 << 14, 132000, 1 << 18, 600000, 1 << 20, 3 << 20):
        for c in (0, 2, 8, 13, 16, 17, 22):
            assert sv.Context.bucket_geometry(n, c) == E.pip_plan(n, c)[:3], (n, c)


def _big_bucket(L, kind):
    """a bucket of 25 L + 1 entries (26 pieces at the cap L: k_fixup's cooperative list), 25 L + 2 where the plan needs an
    even length"""
    n = 25 * L + 1
    if kind in ("dup", "neg"):
        return (n, ("marks", [(n // 2, kind)]))
    if kind == "same":
        return (n, ("pm", n, 0))
    if kind == "cancel":
        return (n + 1, ("pm", (n + 1) // 2, (n + 1) // 2))
    return (n, ("pm", (n + 1) // 2, n // 2))  # "one_left": a copies of P, a - 1 of -P


@pytest.mark.parametrize("L", [32, 128])
@pytest.mark.parametrize("kind", ["dup", "neg", "same", "cancel", "one_left"])
def test_big_split_bucket_with_exceptional_points(L, kind):
    """More than kBigPieces pieces in one bucket, and partials that are degenerate: with nothing but +-P in the bucket
    every piece of two or more entries is, whatever order the sort leaves, so the workgroup's `any_bad` recomputation
    from the entries is certain (L = 32: one MSM of a few thousand terms; L = 128: the hint)."""
    big = _big_bucket(L, kind)
    plan = E.plan_buckets(BN, [big, (L + 1, "distinct")], FILL)
    assert E.pip_plan(plan.n, 16)[5] == 32 and E.pip_plan(plan.n, 16, True)[5] == 128
    assert (big[0] + L - 1) // L > E.BIG_PIECES and plan.lengths[3] == big[0]
    assert plan.expected() == C.msm_pippenger(plan.s, plan.p, 4)
    _both_modes(plan.s, plan.p, c=16)


@pytest.mark.parametrize("L", [32, 128])
def test_small_split_buckets_of_one_point_and_its_negation(L):
    """Split buckets of L + 2 and 2 L + 1 entries (2 and 3 pieces: the lane-per-bucket list) that hold only +-P: a piece
    of such entries leaves a partial that reads as the stored identity without being one, and the stitch must redo the
    bucket rather than skip it.  2 L + 1 copies of P: two such partials and a remainder of one clean entry."""
    specs = E.pm_kinds(L + 2) + E.pm_kinds(2 * L + 1) + [(2 * L + 1, "distinct")]
    plan = E.plan_buckets(BN, specs, FILL)
    assert plan.expected() == C.msm_pippenger(plan.s, plan.p, 4)
    _both_modes(plan.s, plan.p, c=16)


def test_cap_16_bucket_lengths(gpu_ctx):
    """n = 132 000 at c = 16: latency_run_length picks 16.  Whole buckets below and at the cap, split ones above it, and
    24 / 25 full pieces + 1 on either side of kBigPieces, with distinct points and with +-P."""
    n = 132000
    assert E.pip_plan(n, 16)[5] == 16
    specs = [(ln, "distinct") for ln in (15, 16, 17, 33, 16 * 24 + 1, 16 * 25 + 1)]
    specs += E.pm_kinds(16 * 25 + 1) + E.pm_kinds(16 * 24) + E.pm_kinds(33) + E.pm_kinds(18)
    plan = E.plan_buckets(BN, specs, E.fill_digits(n - sum(s[0] for s in specs), 1001, 30001))
    assert plan.n == n
    assert _run(gpu_ctx, plan.s, plan.p, 16) == C.msm_pippenger(plan.s, plan.p, 4) == plan.expected()


@pytest.mark.parametrize("n", [7167, 7168, 7169])
def test_level2_sort_at_the_lds_cap(n, gpu_ctx):
    """every entry in level-1 key 0 of window 0 (1 <= d <= 1024 at c = 16): k_sort_level2's fast path up to kSortCap =
    7 168 items, the global path from 7 169"""
    assert E.pip_plan(n, 16)[3] == 10
    plan = E.plan_buckets(BN, [], E.fill_digits(n, 1, 1023))
    assert _run(gpu_ctx, plan.s, plan.p, 16) == C.msm_pippenger(plan.s, plan.p, 4)


def test_level2_sort_both_paths_in_one_launch(gpu_ctx):
    """key 0 one item above the cap (global path) next to key 1 one item below it (LDS path)"""
    fill = list(E.fill_digits(7169, 1, 1023)) + list(E.fill_digits(7167, 1025, 1023))
    assert E.pip_plan(len(fill), 16)[3] == 10
    plan = E.plan_buckets(BN, [], fill)
    assert _run(gpu_ctx, plan.s, plan.p, 16) == C.msm_pippenger(plan.s, plan.p, 4)


def _crafted():
    return [k for c in (13, 16) for k, _, _ in E.crafted_scalars(BN, c)]


@pytest.mark.parametrize("c", [13, 16])
def test_carry_chains_among_random_terms(c, gpu_ctx):
    """windows whose bits equal B exactly, in runs: the carry into a window is decided further down, and the histogram's
    recoder (for_each_digit) and the partition's (digit_of_window) must agree entry for entry"""
    ks = _crafted()
    assert 150 <= len(ks) <= 300
    n = 2000 + len(ks)
    s = bytearray(C.sample_scalars(0xCA + c, n))
    for i, k in enumerate(ks):  # spread through the random terms
        at = 7 + i * (n // len(ks))
        s[32 * at:32 * at + 32] = O.fe_to_bytes(k)
    p = C.sample_points(0xCB, n)
    assert _run(gpu_ctx, bytes(s), p, c) == C.msm_pippenger(bytes(s), p, 4)


@pytest.mark.parametrize("c", [13, 16])
def test_carry_chains_one_term_each(c, gpu_ctx):
    """every crafted scalar alone, as one-term MSMs of one batch call"""
    import torch

    ks = _crafted()
    p = C.sample_points(0xCC, len(ks))
    ds = _dev(b"".join(O.fe_to_bytes(k) for k in ks))
    dp = _dev(p)
    out = torch.zeros(64 * len(ks), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.msm_pippenger_many_dev([ds.data_ptr() + 32 * i for i in range(len(ks))],
                                   [dp.data_ptr() + 64 * i for i in range(len(ks))], [1] * len(ks), out.data_ptr(), window_bits=c)
    gpu_ctx.sync()
    got = bytes(out.cpu().numpy())
    for i, k in enumerate(ks):
        assert got[64 * i:64 * i + 64] == C.g1_mul(p[64 * i:64 * i + 64], O.fe_to_bytes(k)), (i, hex(k))


@pytest.mark.parametrize("n", [2047, 2048, 2049, 16379])
def test_tile_partition(n, gpu_ctx):
    """one tile less one, one tile, one tile and one, and 8 tiles with a ragged last one (a multiple of 8 tiles takes the
    xcd_tile permutation)"""
    assert (n + E.TILE - 1) // E.TILE == {2047: 1, 2048: 1, 2049: 2, 16379: 8}[n]
    s, p = C.sample_scalars(0xD7, n), C.sample_points(0xD8, n)
    assert _run(gpu_ctx, s, p) == C.msm_pippenger(s, p, 4)
