"""GPU: the pairing decider's lane arithmetic and its two rounds on raw limbs (tests/fq29_model.py sections 4, 4b), through
the two BN254 flavours of tests/devtest/devtest.hip and the host build.  The pieces run one lane per record; the rounds run
one workgroup per record with the real lane exchanges (group8_sum's quad_perm / row_half_mirror butterfly, row_ror:8) in
the order of k_decide_w and k_decide.  Every record is checked against exact integers as on the CPU, and device asm,
device C and host C must return the SAME limbs -- the two float-quotient squeezes included: they round once, in a
fused multiply-add, in every build."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fq29_model as M  # noqa: E402
import test_gpu_field_layer as FL  # noqa: E402

pytestmark = pytest.mark.gpu


class DeciderBuilds(FL.ThreeBuilds):
    def __call__(self, op, a):
        wo = M.ALL_OPS[op][1]
        out = FL._launch(self.asm, op, a, wo)
        M._eq(FL._launch(self.c, op, a, wo), out, "%s: device C against device asm" % op)
        M._eq(self.host(op, a), out, "%s: host C against device asm" % op)
        self.records += len(a)
        return out


@pytest.fixture(scope="module")
def builds():
    b = DeciderBuilds("bn254")
    for lib in (b.asm, b.c):
        for op, (wi, wo) in list(M.DECIDER_OPS.items()) + list(M.ROUND_OPS.items()):
            assert getattr(lib, "dt_%s_io" % op)() == (wi << 16) | wo, op
    return b


def test_decider_pieces_at_their_lazy_bounds(builds):
    """Every piece over the records of the CPU test (test_curve_math_lazy_host.py runs M.decider_suite on the host build:
    residue, value set and model limbs of each record against exact integers).  Here the two device builds must return the
    host's limbs on every record, so each of those properties holds for them as well; the limb shape is checked again."""
    cases = M.decider_cases(M.CURVES["bn254"].fq, 20000)
    assert set(cases) == set(M.DECIDER_OPS)
    for op, inp in sorted(cases.items()):
        assert len(inp) >= 20000, op
        out = builds(op, inp)  # device asm == device C == host C, limb for limb
        if op != "wt_cneg":  # (a limb-wise negation: its output is as lazy as its input)
            for j in range(0, out.shape[1], 9):
                M._assert_norm(out[:, j:j + 9], op)


def test_program_round_on_the_device(builds):
    F = M.CURVES["bn254"].fq
    rows, meta = M.wt_round_cases(F, 2000)
    count, span = M.check_wt_round(F, builds("wt_round", rows), meta)  # limb-equal to the lane-by-lane host emulation inside
    assert set(count) == set(M.WT_VARIANTS) and min(count.values()) >= 2000


def test_team_round_on_the_device(builds):
    F = M.CURVES["bn254"].fq
    rows, meta = M.coop3_round_cases(F, 2000)
    n, span = M.check_coop3_round(F, builds("coop3_round", rows), meta)
    assert n >= 4000
