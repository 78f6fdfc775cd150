"""Child process of tests/test_gpu_ipa_commit_blinded.py: the blinded batch commitment on the route of one MSM per vector,
which a process takes only when SNARKV_IPA_SHARED=0 is set before the library reads it.  Both curves, against the oracle;
prints "per-vector ok" when everything agreed."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ipa_commit_blinded_util as U  # noqa: E402


def main():
    assert os.environ.get("SNARKV_IPA_SHARED") == "0"
    for name in ("bn254", "pallas"):
        cv = U.curve(name)
        rnd = random.Random("per-vector-" + name)
        gb = cv.key_bytes(911, 8)
        dk = cv.dk(gb)
        s64 = cv.point(0x5EED)
        blinds = [0, 1, cv.R - 1, int.from_bytes(b"\x80" * 32, "little"), rnd.randrange(cv.R)]
        for n, m in ((1, 1), (7, 5), (8, 5)):
            vecs = [[rnd.randrange(cv.R) for _ in range(n)] for _ in range(m)]
            got = U.run(cv, dk, s64, vecs, blinds[-m:])
            for a in range(m):
                assert got[64 * a:64 * a + 64] == U.expected(cv, gb, s64, vecs[a], blinds[-m:][a]), (name, n, m, a)
        # the identity as a result: S = -G[0], poly = (blind, 0, ...)
        b = blinds[-1]
        assert U.run(cv, dk, cv.neg(gb[:64]), [[b] + [0] * 7], [b]) == bytes(64)
        assert dk.table_bytes == 0  # this route never builds the window table
        dk.close()
        cv.ctx.close()
    print("per-vector ok")


if __name__ == "__main__":
    main()
