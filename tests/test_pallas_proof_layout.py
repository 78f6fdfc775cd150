"""CPU: the layout pass of the pallas batch reader (host/plonk_ipa_batch.hpp `plonk_ipa_proof_layout`, through the hook
`hp_plonk_ipa_point_offsets`) against the positions at which the oracle's Blake2b transcript actually reads points
while it parses a forged `PlonkProof<Bgh19>`: k in {4, 6, 8}, the three linearizations, one and two instance columns."""
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402
import transcript as T  # noqa: E402


@pytest.fixture(scope="module")
def HP():
    import importlib.util

    from snark_verifier_amd import pallas as PL

    PL.load_library()
    spec = importlib.util.spec_from_file_location("_snarkv_build", os.path.join(ROOT, "snark-verifier_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    h = ctypes.CDLL(b.build_host_driver_pallas())
    h.hp_plonk_ipa_point_offsets.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    return h


@pytest.fixture()
def on_pallas():
    import hostfmt
    import plonk_synth as S

    S.use_curve(PA)
    hostfmt.use_curve(PA)
    yield
    S.use_curve(BN)
    hostfmt.use_curve(BN)


class _Recording(T.Blake2bTranscript):
    def __init__(self, *a):
        super().__init__(*a)
        self.point_reads = []

    def read_ec_point(self):
        self.point_reads.append(self.pos)
        return super().read_ec_point()


@pytest.mark.parametrize("num_instance", [(3,), (2, 3)])
@pytest.mark.parametrize("lin", [None, "WithoutConstant", "MinusVanishingTimesQuotient"])
@pytest.mark.parametrize("k", [4, 6, 8])
def test_point_offsets_are_where_the_oracle_reads_points(HP, on_pallas, k, lin, num_instance):
    import plonk as P
    import plonk_synth as S

    rng = random.Random("layout-%d-%s-%s" % (k, lin, num_instance))
    pr, dl = S.standard_plonk_protocol(rng, k=k, linearization=lin, num_instance=num_instance)
    inst = [[rng.randrange(PA.R) for _ in range(m)] for m in pr["num_instance"]]
    kd = {"g": [rng.randrange(1, PA.R) for _ in range(1 << k)], "h": rng.randrange(1, PA.R), "s": rng.randrange(1, PA.R)}
    proof = P.forge_proof_ipa(pr, inst, kd, lambda stream=b"": T.Blake2bTranscript(PA, stream), rng, dl)
    rec = _Recording(PA, proof)
    P.plonk_proof_read(pr, inst, rec, "bgh19")
    assert rec.pos == len(proof)
    assert len(rec.point_reads) == 12 + 2 * k  # StandardPlonk over Bgh19
    if lin is None:
        assert len(proof) == 32 * (12 + 2 * k + 25)  # 1440 / 1568 / 1696 bytes at k = 4 / 6 / 8
    pb = S.pack_protocol(pr)
    offs, ln = (ctypes.c_uint32 * 64)(), ctypes.c_size_t(0)
    n = HP.hp_plonk_ipa_point_offsets(pb, len(pb), k, offs, 64, ctypes.byref(ln))
    assert n == len(rec.point_reads)
    assert list(offs[:n]) == rec.point_reads
    assert ln.value == len(proof)
    # a smaller buffer is filled as far as it goes, the count is still the whole
    few = (ctypes.c_uint32 * 3)()
    assert HP.hp_plonk_ipa_point_offsets(pb, len(pb), k, few, 3, None) == n and list(few) == rec.point_reads[:3]
