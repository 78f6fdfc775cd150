"""CPU: the reference of the group-transform tests itself (tests/g1_ntt_util.py), not the feature: its Jacobian scalar
multiplication against the oracle's, and its radix-2 transform against the O(n^2) sums of include/snarkv_g1_ntt.h.  These pass
whatever the library does; tests/test_g1_ntt_host.py and tests/test_gpu_g1_ntt.py hold the library against this reference."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import g1_ntt_util as GU  # noqa: E402

CURVES = sorted(GU.CURVES)


@pytest.mark.parametrize("curve", CURVES)
def test_the_references_multiplication_is_the_oracles(curve):
    O = GU.CURVES[curve]
    p, q = GU.random_points(curve, 2, "mul")
    for e in (0, 1, 2, 3, O.R - 1, O.R - 2, (O.R + 1) // 2, (O.R - 1) // 2, 0x1234567 << 200, O.R, O.R + 5):
        assert GU.mul(O, p, e) == O.g1_mul(p, e % O.R), e
    assert GU.mul(O, None, 5) is None
    assert GU.mul(O, q, 2) == O.g1_double(q) and GU.mul(O, q, 3) == O.g1_add(q, O.g1_double(q))


@pytest.mark.parametrize("curve", CURVES)
def test_the_reference_is_the_sum_of_the_header(curve):
    pts = GU.random_points(curve, 4, "definition")
    for direction in (GU.FORWARD, GU.INVERSE):
        assert GU.reference(curve, pts, direction) == GU.definition(curve, pts, direction)
    assert GU.reference(curve, GU.reference(curve, pts, GU.INVERSE), GU.FORWARD) == pts
