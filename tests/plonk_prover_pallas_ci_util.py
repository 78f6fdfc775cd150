"""Shared helpers of the tests of the PLONK prover on pallas with committed instances
(include/snarkv_host_pallas_plonk_prove_ci.h): tests/plonk_prover_pallas_util.py's key, circuits and model prover, extended.

A protocol here carries  instance_committing_key = {bases: the first points of the key's Lagrange basis (tests/g1_ntt_util.py's
inverse transform of the key's g), constant: the key's s}  and lists its instance polynomials among `evaluations` and `queries`:
the shape halo2 gives every proof over IPA.  The model commits each instance polynomial with blind 1 (0 without a constant),
absorbs the points with common_ec_point where the plain session absorbs the scalars, and treats the instance polynomials like
witness polynomials from there on.

Circuits  A and B of plonk_prover_pallas_util with the key added (B's instance also at rotation -1, so that a second query set
          holds it), and `Inst`: a b + c = I_0 + .. + I_(m-1) over m instance columns of any lengths, for the shapes of the
          column itself -- two columns, the whole basis, an empty column, no constant.
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import g1_ntt_util as GU  # noqa: E402
import plonk_prover_pallas_util as PP  # noqa: E402
from plonk_prover_pallas_util import (FORM_COEFFS, FORM_VALUES, I, P, PA, R, S, T, U, TranscriptRefusal, on_pallas,  # noqa: E402,F401
                                      oracle_accepts, pack_acc, proof_length, prove, to_coeffs, Setup)

_LAGRANGE = {}


def lagrange_basis(key):
    """the key's g_lagrange on the CPU: <values, lagrange> = <coefficients, g>"""
    if key.k not in _LAGRANGE:
        _LAGRANGE[key.k] = GU.reference("pallas", key.g, GU.INVERSE)
    return _LAGRANGE[key.k]


def committing_key(key, length, constant=True):
    return {"bases": lagrange_basis(key)[:length], "constant": key.s if constant else None}


def add_key(circuit, rotations=(0,), constant=True, tag="ci"):
    """the circuit under a protocol with the committing key and its instance polynomials evaluated and queried at `rotations`"""
    c = copy.copy(circuit)
    pr = dict(circuit.protocol)
    first = len(pr["preprocessed"])
    extra = [(first + j, rot) for j in range(len(pr["num_instance"])) for rot in rotations]
    pr["evaluations"] = list(pr["evaluations"]) + extra
    pr["queries"] = list(pr["queries"]) + extra
    pr["instance_committing_key"] = committing_key(circuit.key, max(pr["num_instance"] + [0]), constant)
    c.protocol, c.name = pr, "%s-%s" % (circuit.name, tag)
    return c


def circuit_a(k=4):
    return add_key(PP.CircuitA(k))


def circuit_b(k=4):
    return add_key(PP.CircuitB(k), rotations=(0, -1))


class Inst(PP._Circuit):
    """a b + c - (I_0 + .. + I_(m-1)) = 0: m instance columns (polynomials 0 .. m - 1), three witness columns of one phase
    without challenges, nothing preprocessed; degree 2, e = 1, one chunk.  `constant`: the committing key has one (the key's
    s); `key`: False leaves the protocol without a committing key and without instance queries."""

    def __init__(self, k, columns, constant=True, key=True, name=None):
        import random

        self.k, self.n, self.key = k, 1 << k, PP.key_of(k)
        m = len(columns)
        self.name = name or "inst-%s%s%s" % ("-".join(str(len(c)) for c in columns), "" if constant else "-noconst", "" if key else "-nokey")
        rnd = random.Random("inst-%d" % k)
        a = [rnd.randrange(R) for _ in range(self.n)]
        b = [rnd.randrange(R) for _ in range(self.n)]
        rows = [sum(col[i] for col in columns if i < len(col)) % R for i in range(self.n)]
        c = [(rows[i] - a[i] * b[i]) % R for i in range(self.n)]
        self._values = [a, b, c]
        self.pre_coeffs, self.instances = [], [list(col) for col in columns]
        self._draw_blinds("inst", False, [3], 1, 0)
        poly, add, mul, neg = S.poly, S.add, S.mul, S.neg
        gate = add(mul(poly(m), poly(m + 1)), poly(m + 2), *[neg(poly(j)) for j in range(m)])
        witness = [(m, 0), (m + 1, 0), (m + 2, 0)]
        inst = [(j, 0) for j in range(m)] if key else []
        self._finish_protocol({
            "num_instance": [len(col) for col in columns], "num_witness": [3], "num_challenge": [0], "evaluations": inst + witness,
            "queries": inst + witness + [(m + 3, 0)], "quotient": {"chunk_degree": 1, "num_chunk": 1, "numerator": gate},
            "transcript_initial_state": 0x1257})
        if key:
            self.protocol["instance_committing_key"] = committing_key(self.key, max([len(col) for col in columns] + [0]), constant)

    def phase_values(self, ph, challenges):
        return self._values


def _column(k, length, seed):
    import random

    rnd = random.Random("inst-column-%d-%s" % (k, seed))
    return [rnd.randrange(1, R) for _ in range(length)]


def shapes(k=4):
    """name -> circuit: the shapes of the instance columns, every proof of which the oracle must accept"""
    n = 1 << k
    return {
        "A": circuit_a(k),
        "B": circuit_b(k),
        "two-columns": Inst(k, [_column(k, 3, "x"), _column(k, 1, "y")]),
        "whole-basis": Inst(k, [_column(k, n, "w")]),
        "empty-column": Inst(k, [[]]),
        "no-constant": Inst(k, [_column(k, 2, "z")], constant=False),
    }


# ---------------------------------------------------------------- the model prover
def model_prove(circuit):
    """plonk_prover_pallas_util.model_prove for a protocol with or without a committing key -> (proof bytes or None, info)"""
    with on_pallas():
        return _model_prove(circuit)


def _model_prove(c):
    pr, key = c.protocol, c.key
    dom = pr["domain"]
    n = dom.n
    ick = pr.get("instance_committing_key")
    t = T.Blake2bTranscript(PA)

    def write_points(stage, cols, blinds):
        assert len(cols) == len(blinds)
        for col, b in zip(cols, blinds):
            try:
                t.write_ec_point(key.pk.commit(list(col), b))
            except T.TranscriptError as e:
                raise TranscriptRefusal(stage, e) from e

    if pr.get("transcript_initial_state") is not None:
        t.common_scalar(pr["transcript_initial_state"])
    inst_polys = [to_coeffs(list(inst) + [0] * (n - len(inst))) for inst in c.instances]
    inst_blind = 0
    if ick is None:
        for inst in c.instances:
            for v in inst:
                t.common_scalar(v)
    else:
        inst_blind = 1 if ick.get("constant") is not None else 0
        for col in inst_polys:
            try:
                t.common_ec_point(key.pk.commit(list(col), inst_blind))  # not proof bytes: the verifier recomputes them
            except T.TranscriptError as e:
                raise TranscriptRefusal("begin", e) from e
    polys = [list(p) for p in c.pre_coeffs] + inst_polys
    blinds = list(c.pre_blinds) + [inst_blind] * len(c.instances)
    challenges = []
    for ph, (nw, nc) in enumerate(zip(pr["num_witness"], pr["num_challenge"])):
        cols = c.phase_coeffs(ph, list(challenges)) if nw else []
        assert len(cols) == nw
        write_points("phase%d" % ph, cols, c.phase_blinds[ph])
        polys += [list(col) for col in cols]
        blinds += list(c.phase_blinds[ph])
        challenges += [t.squeeze_challenge() for _ in range(nc)]
    h = PP.model_quotient(pr, polys, challenges)
    info = {"h": h, "challenges": challenges, "polys": polys}
    n_chunk = pr["quotient"]["num_chunk"]
    if any(h[n_chunk * n:]):
        info["refused_by"] = "tail"
        return None, info
    chunks = [h[i * n:(i + 1) * n] for i in range(n_chunk)]
    write_points("finish", chunks, c.chunk_blinds)
    z = t.squeeze_challenge()
    info["z"] = z
    for p, rot in pr["evaluations"]:
        t.write_scalar(U.horner(polys[p], dom.rotate_scalar(z, rot), R))
    zn = pow(z, n, R)
    polys.append([sum(pow(zn, i, R) * chunks[i][j] for i in range(n_chunk)) % R for j in range(n)])
    blinds.append(sum(pow(zn, i, R) * c.chunk_blinds[i] for i in range(n_chunk)) % R)
    if PP.numerator_at(pr, polys, challenges, z) != U.horner(polys[-1], z, R) * (zn - 1) % R:
        info["refused_by"] = "identity"
        return None, info
    queries = [(p, dom.rotate_scalar(1, rot), U.horner(polys[p], dom.rotate_scalar(z, rot), R)) for p, rot in pr["queries"]]
    f_blind, p_bar, omega_bar = c.opening_randomness
    draws = iter([f_blind] + list(p_bar) + [omega_bar])
    I.bgh19_create_proof(key.pk, polys, blinds, z, queries, t, lambda: next(draws))
    assert next(draws, None) is None
    return t.finalize(), info


_MODEL = {}


def model_proof(circuit):
    """the model's proof of a circuit, computed once per (circuit, k) and shared"""
    key = (circuit.name, circuit.k)
    if key not in _MODEL:
        _MODEL[key] = model_prove(circuit)
    return _MODEL[key]
