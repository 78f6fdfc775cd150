"""GPU: `snarkv_pallas_g1_decompress` (csrc/decompress_pallas.hip, include/snarkv_pallas_decompress.h) against the
oracle, bit for bit.

The kernel's square root resolves a discrete log in the 2^32-subgroup of Fp bit by bit; how far that log reaches is the
2-adic order of (x^3 + 5)^t.  A uniform draw has order exponent i with probability 2^(i - 33), so the low orders are rare:
the seeded set of 2^15 draws is required -- by assertion, here -- to hold at least two inputs at every exponent from 20
to 32 (32 = x^3 + 5 is not a square)."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pallas_decompress_util as U  # noqa: E402

pytestmark = pytest.mark.gpu
P = U.P


@pytest.fixture(scope="module")
def pctx():
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    yield c
    c.close()


def _check(pctx, encs):
    got, ok = pctx.g1_decompress(b"".join(encs))
    assert len(got) == 64 * len(encs) and len(ok) == len(encs)
    n_ok = 0
    for i, e in enumerate(encs):
        want, wok = U.expected(e)
        assert ok[i] == bool(wok), (i, e.hex())
        assert got[64 * i:64 * i + 64] == want, (i, e.hex())
        n_ok += wok
    return n_ok


def test_decompress_2p15_seeded_pairs_bit_exact(pctx):
    pairs = U.seeded_pairs(3, 1 << 15)
    orders = collections.Counter(U.order_exponent((x * x * x + 5) % P) for x, _ in pairs)
    print("order exponent -> inputs:", sorted(orders.items()))
    for i in range(20, 33):
        assert orders[i] >= 2, (i, orders[i])
    n_ok = _check(pctx, [U.encode(x, par) for x, par in pairs])
    assert n_ok == (1 << 15) - orders[32]


def test_decompress_edges_and_odd_sizes(pctx):
    pairs = U.seeded_pairs(5, 131)
    x_sq = next(x for x, _ in pairs if U.order_exponent((x * x * x + 5) % P) < 32)
    x_ns = next(x for x, _ in pairs if U.order_exponent((x * x * x + 5) % P) == 32)
    edge = [bytes(32), U.encode(0, 1),  # the identity; x = 0 with the parity bit: 5 is not a square
            U.encode(P, 0), U.encode(P, 1), U.encode(P + 7, 0), U.encode((1 << 255) - 1, 1),  # x >= p
            U.encode(x_sq, 0), U.encode(x_sq, 1), U.encode(x_ns, 0), U.encode(x_ns, 1),  # both parities of one x
            U.encode(P - 1, 0), U.encode(P - 1, 1)]  # the generator (-1, 2) and its negative
    assert _check(pctx, edge) == 5
    got, ok = pctx.g1_decompress(edge[6] + edge[7])
    y0, y1 = (int.from_bytes(got[64 * i + 32:64 * i + 64], "little") for i in (0, 1))
    assert ok == [True, True] and y0 + y1 == P and y0 % 2 == 0 and y1 % 2 == 1
    assert pctx.g1_decompress(bytes(32)) == (bytes(64), [True])
    encs = [U.encode(x, par) for x, par in pairs]
    for n in (1, 2, 63, 65, 131):  # n = 1 and sizes that are no multiple of the 64-lane workgroup
        _check(pctx, encs[:n])
    assert pctx.g1_decompress(b"") == (b"", [])


def test_decompress_honours_the_contexts_montgomery_flag():
    """A context with SNARKV_FLAG_MONTGOMERY (`snarkv_pallas_ctx_set_flags`) answers in halo2curves' in-memory form
    (v * 2^256 mod p); the input stays the wire form, the identity and refused encodings stay 64 zero bytes; clearing the
    flag brings the canonical form back."""
    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    c = PL.PallasContext(0)
    try:
        encs = [U.encode(x, par) for x, par in U.seeded_pairs(13, 200)]
        encs += [bytes(32), U.encode(0, 1), U.encode(P, 0), U.encode(P - 1, 0), U.encode(P - 1, 1)]
        c.set_flags(sv.SNARKV_FLAG_MONTGOMERY)
        got, ok = c.g1_decompress(b"".join(encs))
        n_ok = 0
        for i, e in enumerate(encs):
            want, wok = U.expected(e, mont=True)
            assert ok[i] == bool(wok) and got[64 * i:64 * i + 64] == want, (i, e.hex())
            n_ok += wok
        assert 60 < n_ok < 160
        assert got[:64] != U.expected(encs[0])[0] or not ok[0]  # not the canonical form
        c.set_flags(0)
        got, ok = c.g1_decompress(b"".join(encs))
        assert got == b"".join(U.expected(e)[0] for e in encs)
        with pytest.raises(sv.SnarkvError):
            c.set_flags(1 << 7)
    finally:
        c.close()


def test_decompress_abi_arguments_and_the_context_free_form(pctx):
    import ctypes

    import snark_verifier_amd as sv
    from snark_verifier_amd import pallas as PL

    lib = PL.load_library()
    out, ok = ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)
    enc = U.encode(P - 1, 0)
    assert lib.snarkv_pallas_g1_decompress(None, enc, 1, out, ok) == -5  # SNARKV_ERR_ARG
    assert lib.snarkv_pallas_g1_decompress(pctx._h, None, 1, out, ok) == -5
    assert lib.snarkv_pallas_g1_decompress(pctx._h, enc, 1, None, ok) == -5
    assert lib.snarkv_pallas_g1_decompress(pctx._h, enc, 1, out, None) == -5
    assert lib.snarkv_pallas_g1_decompress(pctx._h, None, 0, None, None) == 0  # empty: nothing to do
    assert lib.pallas_g1_decompress(enc, 1, out, ok) == 0
    assert (out.raw, ok.raw) == (U.expected(enc)[0], b"\x01")
    with pytest.raises(sv.SnarkvError):
        pctx.g1_decompress(bytes(31))
