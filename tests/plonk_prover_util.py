"""Shared helpers of the PLONK prover tests (include/snarkv_host_plonk_prove.h): a toy SRS with a known secret, a model of the
whole prover over Python integers (tests/ntt_util.py, tests/quotient_util.py, oracle/transcript.py, oracle/kzg.py through
tests/kzg_multiopen_util.py) that returns proof bytes, and two circuits stated as protocols with satisfying witnesses.

Circuit A  tests/quotient_util.py::Circuit: preprocessed q_mul, q_add, sigma_0..2; one instance column holding a[0] under the
           constraint l_0 (a - I); witness phases [3, 1] (a, b, c | Z), challenges [2, 1] (beta, gamma | y); numerator =
           DistributePowers of the gate, l_0 (1 - Z), the permutation product and the instance constraint.  Degree 4: e = 2,
           three chunks.  No blinding rows: Z wraps to one.  `bad` = "gate" / "copy" are the circuit's broken witnesses.
Circuit B  the constraints of tests/plonk_synth.py::standard_plonk_protocol without its random terms, and with the identity
           side of the second product written out (c + beta delta^2 X + gamma: the synthesised protocol leaves it out, which no
           witness satisfies): last = -6, l_last, l_blind, two Z chained through the first one's value at the last row, a
           random polynomial in the last phase, phases [3, 0, 3], challenges [1, 2, 1].  The fixed columns are zero on the six
           unusable rows, and the witness has random values there.
SHAPES     small protocols, each for one path of the session the two circuits do not take, with the outcome the model and the
           session give: a proof, a refusal by the tail or by the identity at z, the transcript's refusal of an identity
           commitment, the verifier's "Missing query".

The model refuses what the session refuses: a tail in h, and numerator(z) != Q(z) (z^n - 1) -- the only guard where
num_chunk n = N leaves no tail.  `Setup`, `prove` and `check_three_ways` drive a session on the device for the GPU tests.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as O  # noqa: E402
import kzg as K  # noqa: E402
import plonk as P  # noqa: E402
import transcript as T  # noqa: E402
import kzg_multiopen_util as KU  # noqa: E402
import ntt_util as U  # noqa: E402
import plonk_synth as S  # noqa: E402
import quotient_util as QU  # noqa: E402

R = O.R
CURVE = "bn254"
SECRET = KU.SECRET
GWC19, BDFG21 = "gwc19", "bdfg21"
MOS_ID = {GWC19: 0, BDFG21: 1}
TRANSCRIPTS = {"evm": T.EvmTranscript, "poseidon": T.PoseidonTranscript}
TRANSCRIPT_ID = {"evm": 0, "poseidon": 1}
FORM_COEFFS, FORM_VALUES = 0, 1
REFUSAL = "the witness does not satisfy the protocol's constraints"


def commit(coeffs, secret=SECRET):
    """[p(s)] G as a point of the oracle (None: the identity)"""
    return O.g1_from_bytes(KU.mulg(KU.horner(coeffs, secret)))


def to_coeffs(values):
    return U.reference(CURVE, list(values), U.INVERSE)


def srs_bytes(n, secret=SECRET):
    return KU.srs_of(secret, n)


def dk_bytes(secret=SECRET):
    """(g1, g2, s g2) of the toy SRS as the deciding key's bytes"""
    return O.g1_to_bytes(O.G1_GEN), O.g2_to_bytes(O.G2_GEN), O.g2_to_bytes(O.g2_mul(O.G2_GEN, secret))


# ---------------------------------------------------------------- the numerator over integers
def degree(e):
    """constants and challenges 0; polynomials, identity, Lagrange 1; sums the larger, products the sum"""
    tag = e[0]
    if tag in ("const", "challenge"):
        return 0
    if tag in ("identity", "lagrange", "poly"):
        return 1
    if tag in ("neg", "scaled"):
        return degree(e[1])
    if tag == "sum":
        return max(degree(e[1]), degree(e[2]))
    if tag == "prod":
        return degree(e[1]) + degree(e[2])
    assert tag == "dpow"
    d, ds = degree(e[1][0]), degree(e[2])
    for x in e[1][1:]:
        d = max(d + ds, degree(x))
    return d


def extension(e):
    d, ext = max(degree(e), 1), 0
    while (1 << ext) < d:
        ext += 1
    return ext


def evaluate_rows(numerator, cols, x_col, l0_col, challenges, ext, n_ext):
    """`plonk.expr_evaluate` at every row of the extended domain: cols = {poly index: its 2^(k+e) values}; Identity is the X
    column, Lagrange(i) the l_0 column at rotation -i"""
    out = []
    for i in range(n_ext):
        out.append(P.expr_evaluate(
            numerator, lambda s: s % R,
            lambda p: x_col[i] if p[0] == "identity" else l0_col[QU.row_of(i, -p[1], ext, n_ext)],
            lambda q: cols[q[0]][QU.row_of(i, q[1], ext, n_ext)], lambda j: challenges[j], lambda a: -a % R,
            lambda a, b: (a + b) % R, lambda a, b: a * b % R, lambda a, s: a * s % R))
    return out


def model_quotient(pr, polys, challenges):
    """the 2^(k+e) coefficients of numerator / (X^n - 1) on integers, by the extended coset as halo2 does it"""
    k, n = pr["domain"].k, pr["domain"].n
    num = pr["quotient"]["numerator"]
    ext = extension(num)
    n_ext = n << ext
    zeta = QU.zeta(CURVE)
    used = sorted({q[0] for q in P.used_query(num)})
    cols = {p: QU.extend(CURVE, polys[p], k, ext, zeta) for p in used}
    l0 = QU.extend(CURVE, to_coeffs([1] + [0] * (n - 1)), k, ext, zeta)
    x = QU.extend(CURVE, [0, 1] + [0] * (n - 2), k, ext, zeta)
    vals = evaluate_rows(num, cols, x, l0, challenges, ext, n_ext)
    return QU.to_coeffs(CURVE, QU.div_vanishing(CURVE, vals, k, ext, zeta), pow(zeta, -1, R))


# ---------------------------------------------------------------- the model prover
class TranscriptRefusal(T.TranscriptError):
    """the transcript refused a point (the identity) while the model was at `stage`: phase<i> or finish"""

    def __init__(self, stage, cause):
        super().__init__("%s: %s" % (stage, cause))
        self.stage = stage


def numerator_at(pr, polys, challenges, z):
    """numerator(z) as the verifier computes it, from the model's own polynomials: every query is Horner over the coefficient
    list at z w^rot -- the instances', l_i(z) = l_0(z w^-i) and X too.  A query that is neither an instance polynomial nor
    among the protocol's evaluations is the verifier's "Missing query" (verifier/plonk/proof.rs:222-232)."""
    dom = pr["domain"]
    n = dom.n
    l0, x = to_coeffs([1] + [0] * (n - 1)), ([0, 1] + [0] * (n - 2))[:n]
    listed = {tuple(q) for q in pr["evaluations"]}
    first_inst = len(pr["preprocessed"])

    def poly(q):
        if not first_inst <= q[0] < first_inst + len(pr["num_instance"]) and q not in listed:
            raise P.ProtocolError("Missing query %r" % (q,))
        return U.horner(polys[q[0]], dom.rotate_scalar(z, q[1]), R)

    return P.expr_evaluate(
        pr["quotient"]["numerator"], lambda s: s % R,
        lambda p: U.horner(x, z, R) if p[0] == "identity" else U.horner(l0, dom.rotate_scalar(z, -p[1]), R),
        poly, lambda j: challenges[j], lambda a: -a % R, lambda a, b: (a + b) % R, lambda a, b: a * b % R, lambda a, s: a * s % R)


def model_prove(pr, pre_coeffs, instances, phase_fn, mos, transcript, secret=SECRET):
    """The prover of include/snarkv_host_plonk_prove.h on integers.  phase_fn(phase, challenges so far) -> the phase's
    polynomials as coefficient lists.  -> (proof bytes or None, {"h", "challenges", "z", "polys"}).  No proof comes out when
    h has coefficients from num_chunk * n on (info["refused_by"] = "tail") or when numerator(z) != Q(z) (z^n - 1)
    (info["refused_by"] = "identity"; info["unchecked_proof"] has the bytes that would have been written).  An identity
    commitment raises TranscriptRefusal with the stage; a numerator that names an unlisted evaluation raises
    plonk.ProtocolError("Missing query") after the evaluations, where the session's `finish` does."""
    dom = pr["domain"]
    n = dom.n
    t = TRANSCRIPTS[transcript]()

    def write_points(stage, cols):
        for c in cols:
            try:
                t.write_ec_point(commit(c, secret))
            except T.TranscriptError as e:
                raise TranscriptRefusal(stage, e) from e

    if pr.get("transcript_initial_state") is not None:
        t.common_scalar(pr["transcript_initial_state"])
    for inst in instances:
        for v in inst:
            t.common_scalar(v)
    polys = [list(c) for c in pre_coeffs] + [to_coeffs(list(inst) + [0] * (n - len(inst))) for inst in instances]
    challenges = []
    for ph, (nw, nc) in enumerate(zip(pr["num_witness"], pr["num_challenge"])):
        cols = phase_fn(ph, list(challenges)) if nw else []
        assert len(cols) == nw
        write_points("phase%d" % ph, cols)
        polys += [list(c) for c in cols]
        challenges += [t.squeeze_challenge() for _ in range(nc)]
    h = model_quotient(pr, polys, challenges)
    info = {"h": h, "challenges": challenges, "polys": polys}
    n_chunk = pr["quotient"]["num_chunk"]
    if any(h[n_chunk * n:]):
        info["refused_by"] = "tail"
        return None, info
    chunks = [h[i * n:(i + 1) * n] for i in range(n_chunk)]
    write_points("finish", chunks)
    z = t.squeeze_challenge()
    info["z"] = z
    for p, rot in pr["evaluations"]:
        t.write_scalar(U.horner(polys[p], dom.rotate_scalar(z, rot), R))
    zn = pow(z, n, R)
    polys.append([sum(pow(zn, i, R) * chunks[i][j] for i in range(n_chunk)) % R for j in range(n)])
    # the verifier's identity, the session's step 6
    holds = numerator_at(pr, polys, challenges, z) == U.horner(polys[-1], z, R) * (zn - 1) % R
    queries = [(p, dom.rotate_scalar(1, rot), U.horner(polys[p], dom.rotate_scalar(z, rot), R)) for p, rot in pr["queries"]]
    if mos == GWC19:
        v = t.squeeze_challenge()
        for w in KU.gwc19_prove(secret, polys, z, queries, v):
            t.write_ec_point(O.g1_from_bytes(w))
    else:
        mu = t.squeeze_challenge()
        gamma = t.squeeze_challenge()

        def draw(w):
            t.write_ec_point(O.g1_from_bytes(w))
            return t.squeeze_challenge()

        _, _, w_prime = KU.bdfg21_prove(secret, polys, z, queries, mu, gamma, draw)
        t.write_ec_point(O.g1_from_bytes(w_prime))
    if not holds:
        info["refused_by"] = "identity"
        info["unchecked_proof"] = t.finalize()
        return None, info
    return t.finalize(), info


def oracle_accepts(pr, instances, proof, mos, transcript, secret=SECRET):
    """`plonk_proof_read` + `succinct_verify` of the oracle, and lhs = [s] rhs; no byte of the proof is left over"""
    t = TRANSCRIPTS[transcript](proof)
    pf = P.plonk_proof_read(pr, instances, t, mos)
    (lhs, rhs), = P.succinct_verify(O.G1_GEN, pr, instances, pf, mos)
    return rhs is not None and lhs == O.g1_mul(rhs, secret)


# ---------------------------------------------------------------- circuit A
class CircuitA:
    QM, QA, S0, I, A, B, C, Z = 0, 1, 2, 5, 6, 7, 8, 9

    def __init__(self, k, bad=None):
        self.k, self.n, self.bad = k, 1 << k, bad
        c = self.circuit = QU.Circuit(CURVE, k, bad=bad)
        self.fixed_values = [c.qm, c.qa] + c.sigma
        self.pre_coeffs = [to_coeffs(v) for v in self.fixed_values]
        self.instances = [[c.a[0]]]
        poly, add, mul, neg, const = S.poly, S.add, S.mul, S.neg, S.const
        beta, gamma, y = (("challenge", i) for i in range(3))
        l0 = ("lagrange", 0)
        gate = add(mul(poly(self.QM), add(mul(poly(self.A), poly(self.B)), neg(poly(self.C)))),
                   mul(poly(self.QA), add(poly(self.A), poly(self.B), neg(poly(self.C)))))
        left, right = poly(self.Z, 1), poly(self.Z)
        for j in range(3):
            left = mul(left, add(poly(self.A + j), mul(beta, poly(self.S0 + j)), gamma))
            right = mul(right, add(poly(self.A + j), mul(beta, ("scaled", ("identity",), pow(c.delta, j, R))), gamma))
        constraints = [gate, mul(l0, add(const(1), neg(poly(self.Z)))), add(left, neg(right)),
                       mul(l0, add(poly(self.A), neg(poly(self.I))))]
        evaluations = [(p, 0) for p in range(5)] + [(self.A, 0), (self.B, 0), (self.C, 0), (self.Z, 0), (self.Z, 1)]
        self.protocol = {
            "domain": P.Domain(k), "preprocessed": [commit(p) for p in self.pre_coeffs], "num_instance": [1],
            "num_witness": [3, 1], "num_challenge": [2, 1], "evaluations": evaluations, "queries": evaluations + [(10, 0)],
            "quotient": {"chunk_degree": 1, "num_chunk": 3, "numerator": ("dpow", constraints, y)},
            "transcript_initial_state": 0xA11CE, "instance_committing_key": None, "linearization": None,
            "accumulator_indices": [],
        }

    def phase_values(self, ph, challenges):
        c = self.circuit
        if ph == 0:
            return [c.a, c.b, c.c]
        c.beta, c.gamma = challenges[0], challenges[1]
        return [c.z()[0]]

    def phase_coeffs(self, ph, challenges):
        return [to_coeffs(v) for v in self.phase_values(ph, challenges)]


# ---------------------------------------------------------------- circuit B
class CircuitB:
    LAST = -6
    DELTA = 7

    def __init__(self, k, seed="plonk-circuit-b"):
        rnd = random.Random("%s-%d" % (seed, k))
        n = self.n = 1 << k
        self.k = k
        u = self.u = n + self.LAST  # the last row; the rows below it are the active ones
        w = U.omega(CURVE, k)
        a, b, c, inst = [0] * n, [0] * n, [0] * n, [rnd.randrange(R), rnd.randrange(R)]
        qa, qb, qc, qab, qk = ([0] * n for _ in range(5))
        col_i = inst + [0] * (n - 2)
        a[0] = rnd.randrange(R)
        for i in range(u):
            b[i] = b[1] if i == 2 else rnd.randrange(R)
            qa[i], qb[i], qab[i], qk[i], qc[i] = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R), rnd.randrange(R), R - 1
            c[i] = (qa[i] * a[i] + qb[i] * b[i] + qab[i] * a[i] * b[i] + qk[i] + col_i[i]) % R
            if i + 1 < u:
                a[i + 1] = c[i]
        for i in range(u, n):  # the blinding rows
            a[i], b[i], c[i] = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
        self.ids = [[pow(self.DELTA, j, R) * pow(w, i, R) % R for i in range(n)] for j in range(3)]
        self.sigma = [list(x) for x in self.ids]
        for i in range(u - 1):  # (c, i) <-> (a, i + 1)
            self.sigma[2][i], self.sigma[0][i + 1] = self.ids[0][i + 1], self.ids[2][i]
        self.sigma[1][1], self.sigma[1][2] = self.ids[1][2], self.ids[1][1]  # (b, 1) <-> (b, 2)
        self.a, self.b, self.c, self.instances = a, b, c, [inst]
        self.fixed_values = [qa, qb, qc, qab, qk] + self.sigma
        self.pre_coeffs = [to_coeffs(v) for v in self.fixed_values]
        self.blind_z1 = [rnd.randrange(R) for _ in range(n - u - 1)]
        self.blind_z2 = [rnd.randrange(R) for _ in range(n - u - 1)]
        self.random_values = [rnd.randrange(R) for _ in range(n)]
        self.protocol = self._protocol()

    def _protocol(self):
        poly, add, mul, neg, const = S.poly, S.add, S.mul, S.neg, S.const
        q_a, q_b, q_c, q_ab, q_k, s1, s2, s3 = range(8)
        i0, last = 8, self.LAST
        a, b, c, z1, z2, rnd = range(9, 15)
        beta, gamma, alpha = ("challenge", 1), ("challenge", 2), ("challenge", 3)
        l0, llast = ("lagrange", 0), ("lagrange", last)
        lblind = add(*[("lagrange", i) for i in range(last + 1, 0)])
        x = ("identity",)
        gate = add(mul(poly(q_a), poly(a)), mul(poly(q_b), poly(b)), mul(poly(q_c), poly(c)),
                   mul(poly(q_ab), mul(poly(a), poly(b))), poly(q_k), poly(i0))
        active = add(const(1), neg(add(llast, lblind)))
        lhs_p = mul(poly(z1, 1), add(poly(a), mul(beta, poly(s1)), gamma), add(poly(b), mul(beta, poly(s2)), gamma))
        rhs_p = mul(poly(z1), add(poly(a), mul(beta, x), gamma), add(poly(b), mul(beta, ("scaled", x, self.DELTA)), gamma))
        constraints = [
            gate,
            mul(l0, add(const(1), neg(poly(z1)))),
            mul(llast, add(mul(poly(z2), poly(z2)), neg(poly(z2)))),
            mul(l0, add(poly(z2), neg(poly(z1, last)))),
            mul(active, add(lhs_p, neg(rhs_p))),
            mul(active, add(mul(poly(z2, 1), add(poly(c), mul(beta, poly(s3)), gamma)),
                            neg(mul(poly(z2), add(poly(c), mul(beta, ("scaled", x, self.DELTA ** 2)), gamma))))),
        ]
        evaluations = [(a, 0), (b, 0), (c, 0), (a, 1), (c, -1)] + [(i, 0) for i in range(5)] + [(rnd, 0)] + \
                      [(s1, 0), (s2, 0), (s3, 0)] + [(z1, 0), (z1, 1), (z1, last), (z2, 0), (z2, 1)]
        queries = [(a, 0), (b, 0), (c, 0), (a, 1), (c, -1), (z1, 0), (z1, 1), (z1, last), (z2, 0), (z2, 1)] + \
                  [(i, 0) for i in range(5)] + [(s1, 0), (s2, 0), (s3, 0)] + [(15, 0)] + [(rnd, 0)]
        return {
            "domain": P.Domain(self.k), "preprocessed": [commit(p) for p in self.pre_coeffs], "num_instance": [2],
            "num_witness": [3, 0, 3], "num_challenge": [1, 2, 1], "evaluations": evaluations, "queries": queries,
            "quotient": {"chunk_degree": 1, "num_chunk": 3, "numerator": ("dpow", constraints, alpha)},
            "transcript_initial_state": 0xB0B, "instance_committing_key": None, "linearization": None,
            "accumulator_indices": [],
        }

    def z_columns(self, beta, gamma):
        """(z1, z2) on integers: z1 over the columns a, b, z2 over c and started at z1's value at the last row; the rows
        past the last one carry the blinding values"""
        u = self.u
        cols = (self.a, self.b, self.c)

        def run(start, js):
            z = [start]
            for i in range(u):
                num = den = 1
                for j in js:
                    num = num * (cols[j][i] + beta * self.ids[j][i] + gamma) % R
                    den = den * (cols[j][i] + beta * self.sigma[j][i] + gamma) % R
                z.append(z[-1] * num % R * pow(den, -1, R) % R)
            return z

        z1 = run(1, (0, 1))
        z2 = run(z1[u], (2,))
        assert z2[u] == 1
        return z1 + self.blind_z1, z2 + self.blind_z2

    def phase_values(self, ph, challenges):
        if ph == 0:
            return [self.a, self.b, self.c]
        assert ph == 2
        z1, z2 = self.z_columns(challenges[1], challenges[2])
        return [z1, z2, self.random_values]

    def phase_coeffs(self, ph, challenges):
        return [to_coeffs(v) for v in self.phase_values(ph, challenges)]


_MODEL = {}


def model_proof(circuit, mos, transcript):
    """the model's proof of a circuit, computed once per (circuit, scheme, transcript) and shared"""
    key = (type(circuit).__name__, getattr(circuit, "name", None), circuit.k, getattr(circuit, "bad", None), mos, transcript)
    if key not in _MODEL:
        _MODEL[key] = model_prove(circuit.protocol, circuit.pre_coeffs, circuit.instances, circuit.phase_coeffs, mos, transcript)
    return _MODEL[key]


# ---------------------------------------------------------------- the shape catalogue
# Small protocols, each made for one path of the session (host/plonk_prover.hpp) that circuits A and B do not take.  The
# witnesses are drawn from random.Random(name): a model proof is a function of the name.
OUTCOMES = ("proof", "tail", "identity", "transcript@phase0", "transcript@finish", "missing_query")


class Shape:
    """protocol, pre_coeffs, instances, phase_values / phase_coeffs (phase, challenges) -> columns, k, n, and `outcome`:
    what the model and the session make of it.  `form`: how the GPU tests hand the witness over.  `expect`: what the numerator
    compiles to, (l0_col, x_col, first_poly, e)."""

    def __init__(self, name, k, numerator, witness, outcome, expect, num_chunk, pre=(), instances=(), num_witness=None,
                 num_challenge=None, evaluations=None, queries=None, form=FORM_COEFFS):
        self.name, self.k, self.n, self.outcome, self.expect, self.form = name, k, 1 << k, outcome, expect, form
        self.pre_coeffs = [to_coeffs(v) for v in pre]
        self.instances = [list(c) for c in instances]
        num_witness = [len(witness)] if num_witness is None else num_witness
        num_challenge = [0] if num_challenge is None else num_challenge
        self._values, at = [], 0
        for nw, _ in zip(num_witness, num_challenge):  # the phases are the zip of the two lists
            self._values.append([list(c) for c in witness[at:at + nw]])
            at += nw
        assert at == len(witness)
        first = len(pre) + len(instances)
        q_index = first + len(witness)
        if evaluations is None:
            evaluations = [(p, 0) for p in range(len(pre))] + [(first + i, 0) for i in range(len(witness))]
        self.protocol = {
            "domain": P.Domain(k), "preprocessed": [commit(p) for p in self.pre_coeffs], "num_instance": [len(c) for c in instances],
            "num_witness": list(num_witness), "num_challenge": list(num_challenge), "evaluations": list(evaluations),
            "queries": list(evaluations) + [(q_index, 0)] if queries is None else list(queries),
            "quotient": {"chunk_degree": 1, "num_chunk": num_chunk, "numerator": numerator},
            "transcript_initial_state": 0x5EED, "instance_committing_key": None, "linearization": None, "accumulator_indices": [],
        }

    def phase_values(self, ph, challenges):
        return self._values[ph]

    def phase_coeffs(self, ph, challenges):
        return [to_coeffs(v) for v in self._values[ph]]


def product_gate(first, d):
    """p_0 ... p_(d-1) + p_d over the polynomials first .. first + d: no constant, no challenge, no extra column; degree d"""
    return S.add(S.mul(*[S.poly(first + i) for i in range(d)]), S.poly(first + d))


def product_columns(rnd, n, d):
    """d random columns and the one that satisfies the product gate: p_d = -prod"""
    cols = [[rnd.randrange(R) for _ in range(n)] for _ in range(d)]
    last = []
    for i in range(n):
        prod = 1
        for c in cols:
            prod = prod * c[i] % R
        last.append(-prod % R)
    return cols + [last]


def _bump(cols, col, row=0):
    """the same columns with one value off by one: the gate fails at that row"""
    out = [list(c) for c in cols]
    out[col][row] = (out[col][row] + 1) % R
    return out


def _rotated(col, rot):
    """row i -> col[i + rot]: the values of p(w^rot X)"""
    n = len(col)
    return [col[(i + rot) % n] for i in range(n)]


def _shapes():
    out = {}
    poly, add, mul, neg = S.poly, S.add, S.mul, S.neg
    l0, x = ("lagrange", 0), ("identity",)

    def rnd_col(rnd, n):
        return [rnd.randrange(R) for _ in range(n)]

    def put(name, k, numerator, witness, outcome, expect, num_chunk, **kw):
        out[name] = Shape(name, k, numerator, witness(random.Random(name), 1 << k), outcome, expect, num_chunk, **kw)

    def bare(rnd, n):
        return product_columns(rnd, n, 2)

    plain1, plain2, plain3 = (-1, -1, 0, 1), (-1, -1, 0, 2), (-1, -1, 0, 3)
    # a b + c alone: no extra column, no preprocessed polynomial, no instance, no constant; e = 1 and the tail is n long
    put("bare", 3, product_gate(0, 2), bare, "proof", plain1, 1)
    put("bare_k1", 1, product_gate(0, 2), bare, "proof", plain1, 1)
    put("bare_k9", 9, product_gate(0, 2), bare, "proof", plain1, 1)
    put("bare_k10_values", 10, product_gate(0, 2), bare, "proof", plain1, 1, form=FORM_VALUES)
    put("bare_bad", 3, product_gate(0, 2), lambda rnd, n: _bump(bare(rnd, n), 2), "tail", plain1, 1)
    def tail_zero_chunk(rnd, n):
        """a b = p_0 + X^n p_1 and c = -p_0 - s p_1 with s = zeta^2n, the value of X^2n on the extended coset: the numerator
        is p_1 (X^n - s), which the division on the coset turns into h = -X^n p_1 -- a tail, and a first chunk that is zero.
        The tail's verdict comes before the chunks are written: unsatisfied, not the transcript's refusal of the identity."""
        a, b = rnd_col(rnd, n), rnd_col(rnd, n)
        ac, bc, prod = to_coeffs(a), to_coeffs(b), [0] * (2 * n)
        for i in range(n):
            for j in range(n):
                prod[i + j] = (prod[i + j] + ac[i] * bc[j]) % R
        s = pow(QU.zeta(CURVE), 2 * n, R)
        return [a, b, U.reference(CURVE, [(-prod[i] - s * prod[n + i]) % R for i in range(n)], U.FORWARD)]

    put("tail_zero_chunk", 3, product_gate(0, 2), tail_zero_chunk, "tail", plain1, 1)
    put("zero_column", 3, product_gate(0, 2), lambda rnd, n: [rnd_col(rnd, n), [0] * n, [0] * n], "transcript@phase0", plain1, 1)
    put("no_q_query", 3, product_gate(0, 2), bare, "proof", plain1, 1, queries=[(0, 0), (1, 0), (2, 0)])
    put("missing_query", 3, product_gate(0, 2), bare, "missing_query", plain1, 1, evaluations=[(0, 0), (2, 0)])
    # num_chunk n = N: nothing is left for the tail check; the top chunk of a good witness is zero
    put("bare_full", 3, product_gate(0, 2), bare, "transcript@finish", plain1, 2)
    put("bare_full_bad", 3, product_gate(0, 2), lambda rnd, n: _bump(bare(rnd, n), 2), "identity", plain1, 2)
    # the extension
    put("e0_zero", 3, add(poly(0), poly(1)), lambda rnd, n: product_columns(rnd, n, 1), "transcript@finish", (-1, -1, 0, 0), 1)
    put("e0_bad", 3, add(poly(0), poly(1)), lambda rnd, n: [rnd_col(rnd, n), rnd_col(rnd, n)], "identity", (-1, -1, 0, 0), 1)
    put("deg3_two_chunks", 3, product_gate(0, 3), lambda rnd, n: product_columns(rnd, n, 3), "proof", plain2, 2)
    put("deg5_e3", 3, product_gate(0, 5), lambda rnd, n: product_columns(rnd, n, 5), "proof", plain3, 4)
    put("deg5_full", 3, product_gate(0, 5), lambda rnd, n: product_columns(rnd, n, 5), "transcript@finish", plain3, 7)
    put("deg5_all8", 3, product_gate(0, 5), lambda rnd, n: product_columns(rnd, n, 5), "transcript@finish", plain3, 8)

    # one extra column each, and both
    def only_l0(rnd, n):
        a, b = rnd_col(rnd, n), rnd_col(rnd, n)
        b[0] = -a[0] % R
        return [a, b]

    put("only_l0", 3, mul(l0, add(poly(0), poly(1))), only_l0, "proof", (0, -1, 1, 1), 1)

    def only_x(rnd, n):
        w, b = U.omega(CURVE, n.bit_length() - 1), rnd_col(rnd, n)
        return [[pow(w, i, R) * b[i] % R for i in range(n)], b]

    put("only_x", 3, add(poly(0), neg(mul(x, poly(1)))), only_x, "proof", (-1, 0, 1, 1), 1)

    def both(rnd, n):
        a, b = only_l0(rnd, n)
        w = U.omega(CURVE, n.bit_length() - 1)
        return [a, b, [pow(w, i, R) * b[i] % R for i in range(n)]]

    put("both_extras", 3, add(mul(l0, add(poly(0), poly(1))), add(poly(2), neg(mul(x, poly(1))))), both, "proof", (0, 1, 2, 1), 1)

    # phases: none first; witnesses without a challenge; an empty last one; num_witness longer than num_challenge.  One
    # preprocessed column q, the gate q a + b twice under DistributePowers, the second time times the first challenge
    cols = product_columns(random.Random("phases"), 8, 2)
    gate = product_gate(0, 2)
    out["phases"] = Shape("phases", 3, ("dpow", [gate, mul(("challenge", 0), add(poly(2), mul(poly(1), poly(0))))], ("challenge", 2)),
                          cols[1:], "proof", plain1, 1, pre=cols[:1], num_witness=[0, 2, 0, 5], num_challenge=[1, 0, 2])

    # rotations that wrap: w^9 = w at k = 3
    def rot_wrap(rnd, n):
        a = rnd_col(rnd, n)
        a1 = _rotated(a, 1)
        return [a, [-v * v % R for v in a1]]

    wrap = add(mul(poly(0, 1), poly(0, 9)), poly(1))
    put("rot_wrap", 3, wrap, rot_wrap, "proof", plain1, 1, evaluations=[(0, 1), (0, 9), (1, 0)])
    put("eval_lists", 3, wrap, rot_wrap, "proof", plain1, 1, evaluations=[(0, 1), (0, 9), (1, 0), (0, 1)],
        queries=[(1, 0), (2, 0), (0, 9), (0, 1)])

    def rot_extremes(rnd, n):
        a = rnd_col(rnd, n)
        lo, hi = _rotated(a, -512), _rotated(a, 511)
        return [a, [-lo[i] * hi[i] % R for i in range(n)]]

    put("rot_extremes", 3, add(mul(poly(0, -512), poly(0, 511)), poly(1)), rot_extremes, "proof", plain1, 1,
        evaluations=[(0, -512), (0, 511), (1, 0)])

    # instances: an empty column and a full one; short ones under Lagrange polynomials
    rnd = random.Random("instances_0_n")
    full = rnd_col(rnd, 8)
    a, b = rnd_col(rnd, 8), rnd_col(rnd, 8)
    out["instances_0_n"] = Shape("instances_0_n", 3, add(mul(add(poly(2), neg(poly(1))), poly(3)), poly(4)),
                                 [a, b, [-(a[i] - full[i]) * b[i] % R for i in range(8)]], "proof", plain1, 1, instances=[[], full])
    rnd = random.Random("instances_3_1")
    i0, i1 = rnd_col(rnd, 3), rnd_col(rnd, 1)
    a, b = rnd_col(rnd, 8), rnd_col(rnd, 8)
    a[0], a[2], b[0] = i0[0], i0[2], i1[0]
    l2 = ("lagrange", 2)
    num = add(mul(l0, add(poly(2), neg(poly(0)))), mul(l2, add(poly(2), neg(poly(0)))), mul(l0, add(poly(3), neg(poly(1)))))
    out["instances_3_1"] = Shape("instances_3_1", 3, num, [a, b], "proof", (0, -1, 1, 1), 1, instances=[i0, i1])
    return out


SHAPES = _shapes()


# ---------------------------------------------------------------- driving a session on the device (GPU tests)
def to_dev(raw):
    import torch

    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def pack_cols(cols):
    return b"".join(U.pack(c) for c in cols)


class Setup:
    """a circuit's protocol handle, SRS and preprocessed polynomials (None when it has none) on the device"""

    def __init__(self, circuit):
        import torch

        from snark_verifier_amd import host_api as H

        self.circuit = circuit
        self.protocol = H.Protocol(S.pack_protocol(circuit.protocol))
        self.d_srs = to_dev(srs_bytes(circuit.n))
        self.d_pre = to_dev(pack_cols(circuit.pre_coeffs)) if circuit.pre_coeffs else None
        torch.cuda.synchronize()

    def session(self, HP, ctx, mos, transcript):
        return HP.PlonkProver(self.protocol, ctx, self.d_srs, self.d_pre, self.circuit.instances, MOS_ID[mos], TRANSCRIPT_ID[transcript])


def phase_input(circuit, ph, challenges, form):
    """the phase's columns on the device in the given form, or None for a phase without witnesses"""
    if not circuit.protocol["num_witness"][ph]:
        return None
    return to_dev(pack_cols((circuit.phase_values if form == FORM_VALUES else circuit.phase_coeffs)(ph, list(challenges))))


def prove(HP, ctx, setup, mos, transcript, form, phase_columns=None):
    """the whole session -> proof bytes or None.  phase_columns(phase, challenges) -> a device buffer of the phase's columns"""
    import torch

    c = setup.circuit
    given = []
    with setup.session(HP, ctx, mos, transcript) as p:
        challenges = []
        for ph, (nw, _) in enumerate(zip(c.protocol["num_witness"], c.protocol["num_challenge"])):
            d = None
            if nw and phase_columns is not None:
                d = phase_columns(ph, list(challenges))
            elif nw:
                d = phase_input(c, ph, challenges, form)
            if d is not None:
                given.append((d, d.cpu().numpy().tobytes()))
            torch.cuda.synchronize()
            challenges += p.phase(d, form)
        proof = p.finish()
    torch.cuda.synchronize()
    assert all(d.cpu().numpy().tobytes() == raw for d, raw in given)  # the caller's memory is not written
    return proof


def check_three_ways(host_dk, setup, proof, mos, transcript):
    """the proof equals the model's, the oracle accepts it, and snarkv_host_plonk_verify does with the device decider"""
    from snark_verifier_amd import host_api as H

    c = setup.circuit
    want, _ = model_proof(c, mos, transcript)
    assert proof == want
    assert oracle_accepts(c.protocol, c.instances, proof, mos, transcript)
    inst = S.pack_instances(c.instances)
    assert H.plonk_verify(setup.protocol, host_dk, inst, H.pack_proofs([proof]), 1, MOS_ID[mos], TRANSCRIPT_ID[transcript])
    return inst
