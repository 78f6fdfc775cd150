"""CPU: the inputs of the Pippenger edge tests (tests/msm_edge_util.py) are what the GPU tests say they are -- the
launcher's geometry at the sizes the tests use, the planned bucket lengths and level-1 key totals under a restatement of
`for_each_digit`, the crafted GLV halves as the host build of csrc/glv.h returns them, and the planner's expected point
against the plain oracle MSM."""
import random

import pytest

import msm_edge_util as E

CURVES = ["bn254", "pallas"]


def test_launcher_geometry_at_the_sizes_the_tests_use():
    # explicit c = 16 on a GLV build: W = 8, entries = 16 n -- the cap ranges of latency_run_length
    for n, cap in ((3000, 32), (131008, 32), (131009, 16), (132000, 16), (294912, 16), (294913, 32), (589824, 32),
                   (589825, 128), (600000, 128)):
        c, W, B, low, SB, got = E.pip_plan(n, 16)
        assert (c, W, B, got) == (16, 8, 1 << 15, cap), n
        assert E.pip_plan(n, 16, hint=True)[5] == 128
    # a few thousand terms at c = 16: level-1 key 0 of window 0 is the digits 1 .. 1024
    for n in (2000, 7167, 7168, 7169, 14336):
        assert E.pip_plan(n, 16)[3:5] == (10, 32), n
    # from a few thousand terms on the default rule picks among 8, 10, 13, 16: the top window stays populated
    assert {E.pip_plan(n)[0] for n in (2000, 1 << 14, 1 << 16, 1 << 18, 600000, 1 << 20, 1 << 22)} <= {8, 10, 13, 16}
    assert E.pip_plan(1 << 20)[0] == 16 and E.pip_plan(600000)[5] == 128 and E.pip_plan(132000)[5] == 16
    for c in range(2, 23):
        _, W, B, low, SB, _ = E.pip_plan(2000, c)
        assert W * c >= 128 > (W - 1) * c and B == SB << low and low <= 10 and W * SB <= E.MAX_KEYS


def test_recoders_agree_and_rebuild_the_magnitude():
    rnd = random.Random(5)
    for c in (2, 3, 5, 8, 10, 13, 16, 17, 22):
        mags = E.crafted_magnitudes(c) if c >= 8 else []
        mags += [0, 1, (1 << 127) - 1, 1 << 126] + [rnd.getrandbits(127) for _ in range(50)]
        for m in mags:
            ds = E.for_each_digit(m, c)
            assert sum((-d if neg else d) << (c * w) for w, d, neg in ds) == m
            assert all(1 <= d <= 1 << (c - 1) for _, d, _ in ds)
            by_w = {w: (d, neg) for w, d, neg in ds}
            for w in range((128 + c - 1) // c):
                assert E.digit_of_window(m, c, w) == by_w.get(w), (c, hex(m), w)


@pytest.mark.parametrize("name", CURVES)
def test_crafted_halves_are_recovered_and_carry(name):
    cv = E.curve(name)
    lam = cv.lam
    assert (lam * lam + lam + 1) % cv.O.R == 0
    for c in (8, 10, 13, 16, 17):
        got = E.crafted_scalars(cv, c)  # asserts the recovery of every scalar it hands out
        assert len(got) == 8 * len(E.crafted_magnitudes(c))
        B, long_chains = 1 << (c - 1), 0
        for k, k1, k2 in got:
            assert cv.glv_decompose(k) == (k1, k2) and (k1 + k2 * lam - k) % cv.O.R == 0
            assert max(abs(k1), abs(k2)).bit_length() <= E.CRAFT_BITS
            ent = E.scalar_entries(cv, k, c)
            for h, v in enumerate((k1, k2)):
                assert sum((-1 if neg ^ (v < 0) else 1) * d << (c * w) for hh, w, d, neg in ent if hh == h) == abs(v)
            # a carry decided more than one window down: two neighbouring windows of a half hold exactly B
            win = lambda v, w: (abs(v) >> (c * w)) & ((1 << c) - 1)  # noqa: E731
            long_chains += any(win(v, w) == B == win(v, w + 1) for v in (k1, k2) for w in range(1, E.CRAFT_BITS // c))
        assert long_chains >= len(got) // 2


@pytest.mark.parametrize("name", CURVES)
def test_planned_bucket_lengths_under_the_recoder(name):
    cv = E.curve(name)
    specs = [(15, "distinct"), (33, ("marks", [(1, "dup"), (32, "neg")])), (40, ("pm", 20, 20)), (17, ("pm", 9, 8))]
    plan = E.plan_buckets(cv, specs, [1000 + 7 * i for i in range(60)] + [1000] * 3)
    assert plan.n == 15 + 33 + 40 + 17 + 63
    assert [plan.lengths[2 * i + 3] for i in range(4)] == [15, 33, 40, 17] and plan.lengths[1000] == 4
    # the same through the scalar bytes, the GLV split and the recoder: one entry each, half 0, window 0, bucket d - 1
    seen = {}
    for i in range(plan.n):
        k = int.from_bytes(plan.s[32 * i:32 * i + 32], "little")
        (h, w, d, neg), = E.scalar_entries(cv, k, 16)
        assert (h, w, neg) == (0, 0, 0) and d == k == int(plan.digit[i])
        seen[d] = seen.get(d, 0) + 1
    assert seen == plan.lengths
    with pytest.raises(AssertionError):  # one point twice in a bucket the plan calls distinct
        E.plan_buckets(cv, [(5, "distinct")], [1000] * 70, nb=64)


@pytest.mark.parametrize("n", [7167, 7168, 7169])
def test_key_0_totals_at_the_sort_cap(n):
    """n scalars with 1 <= d <= 1024 at c = 16: every entry lands in level-1 key 0 of window 0"""
    cv = E.curve("bn254")
    c, W, B, low, SB, cap = E.pip_plan(n, 16)
    plan = E.plan_buckets(cv, [], E.fill_digits(n, 1, 1023), nb=64)
    keys = {}
    for d, cnt in plan.lengths.items():
        for h, w, dd, _ in E.scalar_entries(cv, d, c):
            key = w * SB + ((dd - 1) >> low)
            keys[key] = keys.get(key, 0) + cnt
    assert keys == {0: n} and (n <= E.SORT_CAP) == (n != 7169) and cap == 32
    # two keys in one launch: 7169 entries in key 0, 7167 in key 1
    two = E.plan_buckets(cv, [], list(E.fill_digits(7169, 1, 1023)) + list(E.fill_digits(7167, 1025, 1023)), nb=64)
    assert E.pip_plan(two.n, 16)[3] == 10
    assert sum(v for d, v in two.lengths.items() if (d - 1) >> 10 == 0) == 7169
    assert sum(v for d, v in two.lengths.items() if (d - 1) >> 10 == 1) == 7167


@pytest.mark.parametrize("name", CURVES)
def test_expected_point_of_a_300_term_plan(name):
    cv = E.curve(name)
    O = cv.O
    specs = [(33, "distinct"), (20, ("marks", [(3, "dup"), (7, "neg")])), (34, ("pm", 17, 17)), (65, ("pm", 33, 32)),
             (40, ("pm", 40, 0)), (9, ("pm", 3, 6))]
    plan = E.plan_buckets(cv, specs, [1000 + 7 * i for i in range(99)])
    assert plan.n == 300
    sc = [int.from_bytes(plan.s[32 * i:32 * i + 32], "little") for i in range(plan.n)]
    pts = [O.g1_from_bytes(plan.p[64 * i:64 * i + 64]) for i in range(plan.n)]
    assert all(O.g1_is_on_curve(q) for q in pts)
    assert plan.expected() == O.g1_to_bytes(O.g1_msm_naive(sc, pts))
    # a plan whose terms cancel altogether is the identity
    assert E.plan_buckets(cv, [(8, ("pm", 4, 4))], [], nb=64).expected() == bytes(64)
    # the host fold of a cycled base equals the term-by-term sum
    rnd = random.Random(2)
    sc = [rnd.randrange(O.R) for _ in range(40)]
    base = cv.base_bytes(16)
    want = O.g1_msm_naive(sc, [O.g1_from_bytes(base[64 * (i % 16):64 * (i % 16) + 64]) for i in range(40)])
    assert E.fold_to_base(cv, sc, 16) == O.g1_to_bytes(want)
