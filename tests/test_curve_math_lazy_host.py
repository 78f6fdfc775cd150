"""CPU: the field and group layer of the device (csrc/fq29.h, fr29.h, fq.h, g1_29.h, glv.h) element by element, on RAW limb
records and at the edges of its lazy-value contract, against exact integers (tests/fq29_model.py): the g++ build of
tests/hosttest/curve_ops.h for BN254 and for pallas.  tests/test_gpu_field_layer.py runs the same cases through the
device builds and requires the same limbs.

  * field operands with limbs at 0, 1, 2^29 - 1, 2^29, +-2^29.8, +-2^30.6 and values next to +-8p, -4p, +-2p, 0, +-p:
    residue, shape, range a*b/2^261 + [0, p), and the nine limbs of the model, for every product-like operation;
  * every k p, k p +- 1 for |k| <= 8 in several limb spellings through fq29_canon_residue / fq29_is_zero_mod_p;
  * accumulators at every corner of the sets that g1_29.h states, through each adder / doubling ONCE: the point, the set
    again, the limb budget of every product inside (an inductive proof-by-test that chains of any length stay legal);
  * P = +-Q and the identity through the fast, careful and skip-identity adders in different spellings of equal points;
  * doubling chains, k P, and that the device test unit really holds the asm multiplier bodies."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fq29_model as M  # noqa: E402

ROOT = M.ROOT
CURVE_NAMES = ["bn254", "pallas"]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_field_operations_at_the_lazy_edges(curve):
    outs, checked = M.field_suite(M.CURVES[curve], M.host_runner(curve), n=50000)
    assert set(checked) == set(M.field_cases(M.CURVES[curve], 50000)) and min(checked.values()) >= 50000


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_column_accumulator_at_the_widest_operands(curve):
    """one operand at 2^29 - 1, the other at +-2^30.6 in every limb 0..7 (limb 8 as small as a value inside (-8p, 8p)
    makes it): the int64 column accumulator must not wrap, in the model and hence in the C it mirrors line by line"""
    F = M.CURVES[curve].fq
    run = M.host_runner(curve)
    peak = 0
    for sa in (1, -1):
        for sb in (1, -1):
            for alt in (0, 1):
                a = M.land([sa * M.MASK * (-1) ** (alt * i) for i in range(8)], 0, 1, F)
                b = M.land([sb * M.W306] * 8, 0, 1, F)
                assert M.budget_ok(F, a, b)
                lim, pk = M.mul_columns(F, [(a, b)])
                peak = max(peak, pk)
                assert run("fq29_mul", np.array([a + b], dtype=np.int32)).tolist()[0] == lim == M.mul_closed(F, [(a, b)])
    print("peak |acc| = 2^%.2f" % np.log2(float(peak)))
    assert peak < 1 << 63


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_every_adder_keeps_the_accumulator_set(curve):
    count = M.closure_suite(M.CURVES[curve], M.host_runner(curve), n_acc=2000)
    assert all(g == c >= 2000 for g, c in count.values())


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_exceptional_additions(curve):
    count = M.exceptional_suite(M.CURVES[curve], M.host_runner(curve), n=2000)
    assert all(g == c >= 2000 for g, c in count.values())


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_doubling_chains_and_scalar_multiplication(curve):
    count = M.chain_suite(M.CURVES[curve], M.host_runner(curve), npts=256)
    assert all(g == c for g, c in count.values()) and count["xyzz29_double_n/254"][0] == 256


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_glv_raw_entry_is_the_byte_entry(curve):
    import ctypes

    rows, ks = M.glv_rows(M.CURVES[curve])
    out = M.host_runner(curve)("glv_decompose", rows)
    lib = M.host_lib(curve)
    buf = ctypes.create_string_buffer(32)
    for k, row in zip(ks[:200], out[:200]):
        lib.hc_glv_decompose(int(k).to_bytes(32, "little"), buf)
        assert buf.raw == row.astype("<i4").tobytes()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_signed_3bit_recoder(curve):
    """glv_w3_digit, the recoder of the segmented MSM's fixed window: digits in [-3, 4] that sum to the magnitude, at the
    edge magnitudes (0, 1, 4, 5, 2^127 - 1, all-0b100, all-0b101) and seeded random ones"""
    n, checked = M.w3_suite(M.host_runner(curve))
    assert n == checked >= 4000


# ---- the pairing decider's lane arithmetic (BN254 only): tests/fq29_model.py sections 4, 4b, 4c
def test_decider_pieces_at_their_lazy_bounds():
    """every piece of SNARKV_RAW_DECIDER_OPS over the operand sets its producers can emit, >= 20 000 records each: residue,
    limb shape, the set the consumers rely on, the model's limbs"""
    checked, mx = M.decider_suite(M.CURVES["bn254"].fq, M.host_runner("bn254"), n=20000)
    assert set(checked) == set(M.DECIDER_OPS) and min(checked.values()) >= 20000
    for name, span in sorted(mx.items()):
        print("%-24s value / p in [%.7f, %.7f]" % ((name,) + span))


def _wt_variants():
    import ctypes

    buf = (ctypes.c_int32 * 128)()
    n = M.host_lib("bn254").hc_wt_variants(buf, 64)
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def test_round_variant_table_is_the_programs():
    """the (kind, flags) table of the round tests is exactly what wt_build_program() emits (WT_FQ2INV is one lane's
    wt_fq2inv, not a round)"""
    assert sorted(M.WT_VARIANTS + [(M.WT_FQ2INV, 0)]) == _wt_variants()


def test_program_round_lane_by_lane_on_corner_operands():
    """one round of k_decide_w emulated lane by lane (csrc/round_emul.h) on every variant, >= 2 000 records each:
    the exact Fq12 / pointwise product, the stored-coefficient invariant, the exact xi copies"""
    F = M.CURVES["bn254"].fq
    rows, meta = M.wt_round_cases(F, 2000)
    count, span = M.check_wt_round(F, M.host_runner("bn254")("wt_round", rows), meta)
    print("stored coefficient / p in [%.7f, %.7f]" % span)
    assert set(count) == set(M.WT_VARIANTS) and min(count.values()) >= 2000


def test_team_round_lane_by_lane_on_corner_operands():
    """one round of k_decide (coop_mul_b) emulated lane by lane: dense, sparse, line-shaped B and squarings"""
    F = M.CURVES["bn254"].fq
    rows, meta = M.coop3_round_cases(F, 2000)
    n, span = M.check_coop3_round(F, M.host_runner("bn254")("coop3_round", rows), meta)
    print("stored coefficient / p in [%.7f, %.7f]" % span)
    assert n >= 4000


def test_g2_prepare_program_stays_inside_its_contracts():
    """integer intervals (units of p) through all levels of g2_prepare_prog.inc, read through the host build: every
    combination fits the fq29_mul2 operand contract, every line coefficient reaches fq29_canon_of_product inside (-p, 2p),
    no level reads a slot that it writes"""
    F = M.CURVES["bn254"].fq
    levels, tasks, slots, prog = M.g2w_program(M.host_lib("bn254"))
    assert (levels, tasks) == (448, 7) and sum(1 for row in prog for t in row if t["used"] and t["dst"] < 0) == 102 * 3
    comb_max, (lo, hi), bad = M.g2w_intervals(F, prog, slots)
    print("largest |combination| = %.4f p; line values in (%.4f p, %.4f p)" % (comb_max, lo, hi))
    assert not bad, bad[:5]
    assert comb_max <= M.G2W_COMB_MAX, "a combination reaches %.3f p: above what g2w_product is tested to" % comb_max
    assert -1 < lo and hi < 2
    # carry-normalised operands within G2W_COMB_MAX p: |limb| < 2^29 and every column of the fused product inside int64
    assert (int(M.G2W_COMB_MAX * F.q) >> 232) + 1 < 1 << 29
    assert M.mul2_column_peak(F, M.G2W_COMB_MAX) < 1 << 63


def _kernel_mads(asm_text, kernel):
    lines = asm_text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN\w*7devtest\d+%sEPKiPii:" % kernel, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return sum(1 for l in lines[start:end] if l.split(";")[0].strip().startswith("v_mad_i64_i32"))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_device_test_unit_holds_the_asm_bodies(curve):
    """The default flavour of tests/devtest/devtest.hip must multiply with the generated asm bodies: at least one
    `v_mad_i64_i32` per partial product in the kernels of mul / mul2 / sqr -- 81 / 162 / 45 operand products plus one
    reduction product per (digit, non-zero limb of the modulus).  Guards against testing the C fallback unawares."""
    spec_b = M.load_build()
    nz = sum(1 for x in M.CURVES[curve].fq.limbs if x != 0)
    need = {"k_fq29_mul": 81 + 9 * nz, "k_fq29_mul2": 162 + 9 * nz, "k_fq29_sqr": 45 + 9 * nz}
    with tempfile.TemporaryDirectory() as d:
        texts = {}
        for fl in (curve + "_asm", curve + "_c"):
            out = os.path.join(d, fl + ".s")
            subprocess.run([spec_b.HIPCC] + spec_b.FLAGS + spec_b.DEVTEST_FLAVOURS[fl] +
                           ["-S", "--cuda-device-only", "-o", out, spec_b.devtest_sources()[0]], check=True, capture_output=True)
            texts[fl] = open(out).read()
    for k, n in need.items():
        got = _kernel_mads(texts[curve + "_asm"], k)
        assert got >= n, (k, got, n)
        assert _kernel_mads(texts[curve + "_c"], k) != got, "the two flavours of %s are the same code" % k
