"""CPU: the numerator compiler of the PLONK prover (snark-verifier_amd/host/plonk_compile.hpp) through its hook in
libsnarkv_hosttest.so.  The numerators of the two circuits of tests/plonk_prover_util.py and of 24 random protocols
(tests/plonk_synth.py::random_protocol) are compiled, the programs run row by row with tests/quotient_util.py::interpret over
random columns, and every row is compared with oracle/plonk.py::expr_evaluate over the same columns: Identity is the X column,
Lagrange(i) the l_0 column at rotation -i.  Then every refusal, each on a protocol made for it."""
import copy
import ctypes
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hostfmt  # noqa: E402
import plonk_prover_util as PU  # noqa: E402
import plonk_synth as S  # noqa: E402
import quotient_util as QU  # noqa: E402

R = PU.R
INVALID_PROTOCOL = -12
REGS, MAX_INSTR, MAX_CONSTS = 16, 4096, 1024


class Refused(Exception):
    pass


@pytest.fixture(scope="module")
def lib():
    return hostfmt.load_host_lib()


def compile_(lib, pr, whole=False):
    """-> the compiled numerator as a dict; raises Refused with the compiler's message"""
    raw = S.pack_protocol(pr)
    info = (ctypes.c_uint32 * 10)()
    prog, consts = ctypes.create_string_buffer(16 * MAX_INSTR), ctypes.create_string_buffer(32 * MAX_CONSTS)
    slots, err = (ctypes.c_uint32 * (2 * MAX_CONSTS))(), ctypes.create_string_buffer(512)
    lib.hd_plonk_compile.restype = ctypes.c_int
    lib.hd_plonk_compile.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                                     ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    rc = lib.hd_plonk_compile(raw, len(raw), int(whole), info, prog, len(prog), consts, len(consts), slots, len(slots), err, len(err))
    if rc == INVALID_PROTOCOL:
        raise Refused(err.value.decode())
    assert rc == 1, rc
    e, degree, n_cols, n_instr, n_consts, l0, x, first_poly, n_slots, regs = info
    return {"e": e, "degree": degree, "n_cols": n_cols, "instrs": QU.decode(prog.raw[:16 * n_instr]),
            "consts": QU.unpack(consts.raw[:32 * n_consts]), "l0_col": l0 - 1, "x_col": x - 1, "first_poly": first_poly,
            "slots": [(slots[2 * i], slots[2 * i + 1]) for i in range(n_slots)], "regs": regs}


def check_against_the_oracle(c, pr, k, seed):
    """the program over random columns == expr_evaluate over the same columns, at every row"""
    rnd = random.Random("plonk-compile-%s" % (seed,))
    e = c["e"]
    n_ext = 1 << (k + e)
    cols = [[rnd.randrange(R) for _ in range(n_ext)] for _ in range(c["n_cols"])]
    challenges = [rnd.randrange(R) for _ in range(sum(pr["num_challenge"]))]
    consts = list(c["consts"])
    for at, ch in c["slots"]:
        assert consts[at] == 0
        consts[at] = challenges[ch]
    assert len({at for at, _ in c["slots"]}) == len(c["slots"]) == len({ch for _, ch in c["slots"]})
    got = QU.interpret(PU.CURVE, cols, k, e, c["instrs"], consts)
    by_poly = {p: cols[c["first_poly"] + p] for p in range(c["n_cols"] - c["first_poly"])}
    want = PU.evaluate_rows(pr["quotient"]["numerator"], by_poly, cols[c["x_col"]] if c["x_col"] >= 0 else None,
                            cols[c["l0_col"]] if c["l0_col"] >= 0 else None, challenges, e, n_ext)
    assert got == want
    assert c["degree"] == PU.degree(pr["quotient"]["numerator"]) and e == PU.extension(pr["quotient"]["numerator"])
    assert max(i[1] for i in c["instrs"]) + 1 == c["regs"] <= REGS


def test_circuit_a(lib):
    a = PU.CircuitA(4)
    for whole in (False, True):
        c = compile_(lib, a.protocol, whole)
        assert (c["degree"], c["e"], c["first_poly"], c["n_cols"]) == (4, 2, 2, 12) and (c["l0_col"], c["x_col"]) == (0, 1)
        assert sorted(ch for _, ch in c["slots"]) == [0, 1, 2]
        check_against_the_oracle(c, a.protocol, 3, "A")


def test_circuit_b(lib):
    b = PU.CircuitB(4)
    c = compile_(lib, b.protocol, True)
    assert (c["degree"], c["e"], c["first_poly"], c["n_cols"]) == (4, 2, 2, 17)
    assert sorted(ch for _, ch in c["slots"]) == [1, 2, 3]  # theta is not used
    check_against_the_oracle(c, b.protocol, 3, "B")


@pytest.mark.parametrize("seed", range(24))
def test_random_protocols(lib, seed):
    pr, _ = S.random_protocol(random.Random(7000 + seed), None)
    c = compile_(lib, pr)
    assert c["degree"] <= 3 and c["regs"] <= 4 and len(c["instrs"]) <= 17
    if seed == 22:  # a bare leaf: leaf + 0
        assert len(c["instrs"]) == 1 and PU.degree(pr["quotient"]["numerator"]) <= 1
    check_against_the_oracle(c, pr, 3, seed)


# ---------------------------------------------------------------- the refusals
def _with(**changes):
    pr = copy.copy(PU.CircuitA(4).protocol)
    pr["quotient"] = dict(pr["quotient"])
    for key, v in changes.items():
        if key in ("numerator", "chunk_degree", "num_chunk"):
            pr["quotient"][key] = v
        else:
            pr[key] = v
    return pr


def _refusal(lib, pr, whole=True):
    with pytest.raises(Refused) as e:
        compile_(lib, pr, whole)
    return str(e.value)


def test_the_limits_are_named(lib):
    ch, one = ("challenge", 0), ("const", 1)
    deep = ("sum", one, ch)
    for _ in range(REGS + 1):  # every level holds its accumulator while the scalar below it is computed
        deep = ("dpow", [("sum", one, ch), ("sum", one, ch)], deep)
    assert "SNARKV_QUOT_REGS" in _refusal(lib, _with(numerator=deep))
    long_ = ("dpow", [("sum", one, ch)] * (MAX_INSTR // 2 + 2), ch)
    assert "SNARKV_QUOT_MAX_INSTR" in _refusal(lib, _with(numerator=long_))
    many = ("dpow", [("const", 5 + i) for i in range(MAX_CONSTS + 1)], ch)
    assert "SNARKV_QUOT_MAX_CONSTS" in _refusal(lib, _with(numerator=many))
    # the three just below their limits compile
    ok = ("sum", one, ch)
    for _ in range(REGS - 2):  # at the innermost level: the outer accumulators, its own, the scalar and a term
        ok = ("dpow", [("sum", one, ch), ("sum", one, ch)], ok)
    assert compile_(lib, _with(numerator=ok, num_chunk=1), True)["regs"] == REGS
    assert len(compile_(lib, _with(numerator=("dpow", [("sum", one, ch)] * (MAX_INSTR // 2), ch), num_chunk=1), True)["instrs"]) <= MAX_INSTR
    assert len(compile_(lib, _with(numerator=("dpow", [("const", 5 + i) for i in range(MAX_CONSTS - 1)], ch), num_chunk=1), True)["consts"]) == MAX_CONSTS


def test_the_extension_is_at_most_8(lib):
    assert "e > 8" in _refusal(lib, _with(numerator=S.mul(*[S.poly(6)] * 257)))
    c = compile_(lib, _with(numerator=S.mul(*[S.poly(6)] * 256), num_chunk=255), True)
    assert (c["degree"], c["e"]) == (256, 8)


def test_lagrange_indices_outside_the_rotation_field(lib):
    for i in (513, -512, 1 << 20):
        assert "Lagrange" in _refusal(lib, _with(numerator=("lagrange", i)))
    for i in (512, -511):
        c = compile_(lib, _with(numerator=("lagrange", i), num_chunk=1), True)
        assert len(c["instrs"]) == 1 and c["l0_col"] == 0 and c["x_col"] == -1
    assert "rotation" in _refusal(lib, _with(numerator=S.poly(6, 512)))


def test_the_protocol_level_refusals(lib):
    a = PU.CircuitA(4).protocol
    assert "linearization" in _refusal(lib, _with(linearization="WithoutConstant"))
    assert "linearization" in _refusal(lib, _with(linearization="MinusVanishingTimesQuotient"))
    assert "instance_committing_key" in _refusal(lib, _with(instance_committing_key={"bases": [a["preprocessed"][0]], "constant": None}))
    assert "chunk_degree" in _refusal(lib, _with(chunk_degree=2))
    assert "query of an instance polynomial" in _refusal(lib, _with(queries=a["queries"] + [(5, 0)]))
    assert "evaluation of an instance polynomial" in _refusal(lib, _with(evaluations=a["evaluations"] + [(5, 1)]))
    assert "past the quotient's index 10" in _refusal(lib, _with(queries=a["queries"] + [(11, 0)]))
    assert "past the quotient's index 10" in _refusal(lib, _with(evaluations=a["evaluations"] + [(10, 0)]))
    assert "past the quotient's index 10" in _refusal(lib, _with(numerator=S.add(S.poly(6), S.poly(10))))
    assert "past the quotient's index 10" in _refusal(lib, _with(numerator=S.poly(10)), whole=False)
    assert "rotation 0 alone" in _refusal(lib, _with(queries=a["queries"] + [(10, 1)]))
    assert "num_chunk" in _refusal(lib, _with(num_chunk=5))
    # the numerator alone is compiled whatever the rest of the protocol says
    assert compile_(lib, _with(chunk_degree=2, linearization="WithoutConstant"))["degree"] == 4
