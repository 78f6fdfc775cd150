"""GPU: the cases of tests/test_curve_math_lazy_host.py through the device builds of the same operations
(tests/devtest/devtest.hip: one kernel per operation, one lane per record): for BN254 and pallas, the flavour with the
generated asm multiplier bodies and the flavour with the plain-C bodies (-DSNARKV_NO_SMAD_ASM).  Every record's output is
checked against exact integers exactly as on the CPU (residue, shape, range, the model's limbs, the point, the set), and
the three builds -- host C, device C, device asm -- must return the SAME limbs: they implement one column schedule.

The device is opened only through torch allocations and the test library's launchers."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fq29_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
CURVE_NAMES = ["bn254", "pallas"]
_LIBS = {}


def _dev_lib(flavour):
    """the flavour `build()` left next to devtest.hip, rebuilt here when stale and hipcc is at hand"""
    if flavour in _LIBS:
        return _LIBS[flavour]
    import torch  # noqa: F401  (first: the library must bind to the HIP runtime torch brings)

    b = M.load_build()
    so = b.devtest_lib(flavour)
    if os.path.exists(b.HIPCC):
        b.build_devtest(flavour)
    assert os.path.exists(so), "%s is missing: run build()" % so
    lib = ctypes.CDLL(so)
    lib.dt_curve.restype = ctypes.c_char_p
    assert lib.dt_curve().decode() == flavour.split("_")[0]
    assert lib.dt_asm_bodies() == (1 if flavour.endswith("_asm") else 0)
    for op, (wi, wo) in M.OPS.items():
        assert getattr(lib, "dt_%s_io" % op)() == (wi << 16) | wo, op
    _LIBS[flavour] = lib
    return lib


def _launch(lib, name, a, words_out):
    import torch

    a = np.ascontiguousarray(a, dtype=np.int32)
    din = torch.from_numpy(a).cuda()
    dout = torch.zeros((len(a), words_out), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    status = getattr(lib, "dt_" + name)(ctypes.c_void_p(din.data_ptr()), ctypes.c_void_p(dout.data_ptr()), len(a))
    assert status == 0, "%s: HIP status %d" % (name, status)
    return dout.cpu().numpy()


class ThreeBuilds:
    """run(op, records): the device asm flavour's output, after the device C flavour and the host C build have been
    required to give the same limbs for every record"""

    def __init__(self, curve):
        self.curve = curve
        self.asm, self.c = _dev_lib(curve + "_asm"), _dev_lib(curve + "_c")
        self.host = M.host_runner(curve)
        self.records = 0

    def __call__(self, op, a):
        assert len(a) <= 100000
        wo = M.OPS[op][1]
        out = _launch(self.asm, op, a, wo)
        M._eq(_launch(self.c, op, a, wo), out, "%s %s: device C against device asm" % (self.curve, op))
        M._eq(self.host(op, a), out, "%s %s: host C against device asm" % (self.curve, op))
        self.records += len(a)
        return out


@pytest.fixture(scope="module", params=CURVE_NAMES)
def builds(request):
    return ThreeBuilds(request.param)


def test_field_operations_at_the_lazy_edges(builds):
    C = M.CURVES[builds.curve]
    outs, checked = M.field_suite(C, builds, n=50000)
    assert set(checked) == set(M.field_cases(C, 50000)) and min(checked.values()) >= 50000


def test_every_adder_keeps_the_accumulator_set(builds):
    count = M.closure_suite(M.CURVES[builds.curve], builds, n_acc=2000)
    assert all(g == c >= 2000 for g, c in count.values())


def test_exceptional_additions(builds):
    count = M.exceptional_suite(M.CURVES[builds.curve], builds, n=2000)
    assert all(g == c >= 2000 for g, c in count.values())


def test_doubling_chains_and_scalar_multiplication(builds):
    count = M.chain_suite(M.CURVES[builds.curve], builds, npts=256)
    assert all(g == c for g, c in count.values()) and count["xyzz29_double_n/254"][0] == 256


def test_quad_doubling_equals_the_plain_one(builds):
    """jac29_double_quad (three lanes of a quad share the products, exchanged by DPP) next to jac29_double on the same
    inputs: equal limb for limb, in both flavours, and equal to the host's jac29_double"""
    C = M.CURVES[builds.curve]
    rows = M.jac_corner_rows(C, 2000)
    want = builds("jac29_double", rows)
    for lib in (builds.asm, builds.c):
        out = _launch(lib, "jac29_double_quad", rows[:, :27], 54)
        M._eq(out[:, 27:], want, builds.curve + " jac29_double in the quad kernel")
        M._eq(out[:, :27], want, builds.curve + " jac29_double_quad against jac29_double")


def test_glv_split_on_the_device_is_the_hosts(builds):
    rows, ks = M.glv_rows(M.CURVES[builds.curve])
    out = builds("glv_decompose", rows)  # bit-equal across the three builds inside
    assert len(out) == len(ks) >= 4000


def test_signed_3bit_recoder_on_the_device(builds):
    """the cases of test_signed_3bit_recoder (tests/test_curve_math_lazy_host.py); bit-equal across the three builds inside"""
    n, checked = M.w3_suite(builds)
    assert n == checked >= 4000
