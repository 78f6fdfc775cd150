"""CPU: the C ABI of the lookup calls (include/snarkv_lookup.h): the header is strict C99, both device libraries export every
declared name and only their own, the ctypes table of snark_verifier_amd.lookup lists exactly those names and shares none with
the other tables, the sizes the header states are the module's, and every refusal of the header comes back with its code, in
the header's order, each overlap on its own, without a device (the argument checks come before any HIP call; the context is a
fake struct)."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "snarkv_lookup.h")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import abi_util as AU  # noqa: E402
import bn254 as BN  # noqa: E402
import pallas as PA  # noqa: E402

FIELD = {"bn254": BN.R, "pallas": PA.R}
CALLS = ["poly_sort_dev", "lookup_permute_dev", "lookup_product_dev"]


def test_header_is_strict_c99():
    AU.assert_strict_c99(HDR)


def test_both_libraries_export_the_declared_names_and_the_table_lists_them():
    import snark_verifier_amd as sv
    from snark_verifier_amd import lookup
    from snark_verifier_amd import pallas as PL

    want = sorted(p + c for p in ("snarkv_", "snarkv_pallas_") for c in CALLS)
    assert AU.declared(HDR) == want == sorted(lookup.SIGNATURES)
    assert not set(want) & AU.other_tables(lookup)
    for hdr in os.listdir(INC):  # no other header declares them
        if hdr != "snarkv_lookup.h":
            assert not set(want) & set(AU.declared(os.path.join(INC, hdr))), hdr
    bn, pa = sv.load_library(), PL.load_library()
    for name in want:
        assert hasattr(pa if "pallas" in name else bn, name), name
        assert not hasattr(bn if "pallas" in name else pa, name), name
    for fn in ("sort_dev", "permute_dev", "product_dev"):
        assert callable(getattr(sv.lookup, fn))


def test_the_sizes_of_the_header_are_the_modules(tmp_path):
    from snark_verifier_amd import lookup as L

    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "snarkv_lookup.h"\nint main(void) {\n'
                   '  printf("%lu %lu\\n", (unsigned long)SNARKV_LOOKUP_TILE, (unsigned long)SNARKV_LOOKUP_SCAN_BLOCK);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, check=True).stdout
    assert [int(v) for v in out.split()] == [L.TILE, L.SCAN_BLOCK] == [1024, 1024]
    assert L.SCAN_LEVEL_BLOCK == 1024 and L.STATUS_BYTES == 16


def test_every_refusal_comes_without_a_device():
    """(a correct call is never made here: a fake context must not reach the runtime)"""
    import snark_verifier_amd as sv
    from snark_verifier_amd import lookup as L

    ARG, ENC, EMPTY, LENGTH = sv.SNARKV_ERR_ARG, sv.SNARKV_ERR_ENCODING, sv.SNARKV_ERR_EMPTY, sv.SNARKV_ERR_LENGTH
    for pallas, curve in ((False, "bn254"), (True, "pallas")):
        a = L.api(pallas)
        r = FIELD[curve]
        ctx = AU.FakeCtx(device=0)
        pc = ctypes.addressof(ctx)
        fe = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
        n = 100
        col = 32 * n
        big = (1 << 30) + 1
        # device addresses are only compared here, never followed
        IN, WORK, OUT, TABLE, PI, PT, ST, Z, TOT, START = ((1 << 44) * i for i in range(1, 11))

        def overlap(rc):
            return rc == ARG and "overlap" in a.last_error()

        # ---- sort
        def so(c=pc, i=IN, nn=n, w=WORK, o=OUT):
            return a.poly_sort_dev(c, i, nn, w, o)

        assert so(c=None) == ARG and so(i=None) == ARG and so(w=None) == ARG and so(o=None) == ARG
        assert so(i=IN + 8) == ARG and so(w=WORK + 4) == ARG and so(o=OUT + 8) == ARG  # 16-byte alignment
        for o in (IN + 32, IN - 32, IN + col - 32, IN - col + 32):  # out: the input itself or disjoint from it
            assert overlap(so(o=o)), o - IN
        for w in (IN, IN + 32, IN + col - 32, IN - col + 32):  # work: disjoint from the input ...
            assert overlap(so(w=w)), w - IN
        for w in (OUT, OUT + 32, OUT + col - 32, OUT - col + 32):  # ... and from out
            assert overlap(so(w=w)), w - OUT
        assert overlap(so(o=IN, w=IN + 32))  # in place: work still disjoint
        assert so(nn=0) == EMPTY and so(nn=big) == LENGTH
        assert so(o=IN, nn=0) == EMPTY and so(o=IN, nn=big) == LENGTH  # in place is allowed, so it reaches the length checks
        # the order: arguments, then empty, then the length
        assert so(i=None, nn=0) == ARG and so(o=OUT + 8, nn=big) == ARG and overlap(so(w=IN + 32, nn=big))

        # ---- permute
        def pe(c=pc, i=IN, t=TABLE, uu=n, w=WORK, pi=PI, pt=PT, st=ST):
            return a.lookup_permute_dev(c, i, t, uu, w, pi, pt, st)

        for k in ("c", "i", "t", "w", "pi", "pt", "st"):
            assert pe(**{k: None}) == ARG, k
        for k, v in (("i", IN), ("t", TABLE), ("w", WORK), ("pi", PI), ("pt", PT), ("st", ST)):
            assert pe(**{k: v + 8}) == ARG, k
        # the input, the table, work (2u elements) and the two outputs: pairwise disjoint, each pair on its own
        bufs = {"i": (IN, col), "t": (TABLE, col), "w": (WORK, 2 * col), "pi": (PI, col), "pt": (PT, col)}
        for x, (bx, sx) in bufs.items():
            for y, (by, sy) in bufs.items():
                if x != y:
                    for at in (by, by + 32, by + sy - 32, by - sx + 32):
                        assert overlap(pe(**{x: at})), (x, y, at - by)
        for y in ("w", "pi", "pt"):  # the status lies in nothing the call writes
            by, sy = bufs[y]
            assert overlap(pe(st=by)) and overlap(pe(st=by + sy - 16)), y
        assert pe(uu=0) == EMPTY and pe(uu=big) == LENGTH
        # the order: arguments, then empty, then the length (columns of no rows overlap nothing)
        assert pe(t=None, uu=0) == ARG and pe(pt=PI, uu=0) == EMPTY and overlap(pe(pt=PI + 32, uu=big)) and pe(st=ST + 4, uu=big) == ARG

        # ---- product
        def pr(c=pc, p=IN, nn=n, npolys=4, ia=0, it=1, ipa=2, ipt=3, b=fe(3), g=fe(5), s=START, w=WORK, z=Z, tot=TOT):
            return a.lookup_product_dev(c, p, nn, npolys, ia, it, ipa, ipt, b, g, s, w, z, tot)

        assert pr(c=None) == ARG and pr(p=None) == ARG and pr(w=None) == ARG and pr(z=None) == ARG
        assert pr(b=None) == ARG and pr(g=None) == ARG
        assert pr(p=IN + 8) == ARG and pr(w=WORK + 8) == ARG and pr(z=Z + 4) == ARG and pr(s=START + 8) == ARG and pr(tot=TOT + 8) == ARG
        assert pr(s=None, nn=0) == EMPTY and pr(tot=None, nn=0) == EMPTY  # start and total may be null
        for k in ("ia", "it", "ipa", "ipt"):  # an index >= n_polys
            assert pr(**{k: 4}) == ARG and "index" in a.last_error(), k
            assert pr(**{k: 0xFFFFFFFF}) == ARG, k
        # a buffer the call writes and a column it names: the column at index 3 of 5, each output on its own
        named = IN + 3 * col
        for k, size in (("w", 2 * col), ("z", col), ("tot", 32)):
            for at in (named, named + 32, named + col - 32, named - size + 32):
                assert overlap(pr(npolys=5, **{k: at})), (k, at - named)
            assert pr(npolys=5, ia=0, it=0, ipa=0, ipt=0, b=fe(r), **{k: named}) == ENC  # a column not named is free
        # work, z and the total are disjoint
        for at in (WORK, WORK + 32, WORK + 2 * col - 32, WORK - col + 32):
            assert overlap(pr(z=at)), at - WORK
        assert overlap(pr(tot=WORK)) and overlap(pr(tot=WORK + 2 * col - 32)) and overlap(pr(tot=Z)) and overlap(pr(tot=Z + col - 32))
        # the start value lies in none of the three, and may lie in a column
        assert overlap(pr(s=WORK + 32)) and overlap(pr(s=Z + col - 32)) and overlap(pr(s=TOT))
        assert pr(s=IN + 32, b=fe(r)) == ENC
        assert pr(b=fe(r)) == ENC and pr(g=fe(r)) == ENC and pr(g=b"\xff" * 32) == ENC and pr(b=fe(r - 1), g=fe(0), nn=0) == EMPTY
        assert pr(nn=0) == EMPTY and pr(npolys=0) == EMPTY and pr(nn=big) == LENGTH
        # the order: arguments, then the encoding, then empty, then the length
        assert pr(ia=9, b=fe(r)) == ARG and overlap(pr(z=WORK, g=fe(r))) and pr(p=None, nn=0) == ARG
        assert pr(b=fe(r), nn=0) == ENC and pr(g=fe(r), npolys=0) == ENC and pr(b=fe(r), nn=big) == ENC
        assert pr(npolys=0, nn=big) == EMPTY and pr(nn=0, ia=9) == ARG
