"""A Python prover of the two KZG multi-open schemes, used as the expectation of the device provers
(include/snarkv_kzg_multiopen.h).  Under a toy secret s a commitment is [p(s)] G, so every output point follows from Horner
values at s, Lagrange values of the r_i at s and z', and one scalar multiplication: no polynomial is ever divided here, which
keeps the expectation independent of the device's route.  tests/test_kzg_multiopen_model.py pins these outputs with the
verifiers of oracle/kzg.py.

Also the host-side plan of csrc/kzg_multiopen_plan.h in Python integers, number for number: sets, polynomial order, the
scalars of the linear combinations, the coefficients of r, and after z' the scalars of L, its constant and Z_1(z').
TEST INFRASTRUCTURE ONLY."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as O  # noqa: E402
import coracle as C  # noqa: E402
import kzg as K  # noqa: E402

R = O.R
GWC19, BDFG21 = 0, 1
_GEN = O.g1_to_bytes(O.G1_GEN)


def inv(a):
    return pow(a % R, -1, R)


def horner(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def mulg(k):
    """[k] G as 64 bytes; the identity is 64 zero bytes"""
    k %= R
    return b"\x00" * 64 if k == 0 else C.g1_mul(_GEN, O.fe_to_bytes(k))


def srs(s, n):
    """[s^i] G, i < n, packed"""
    out, p = [], 1
    for _ in range(n):
        out.append(mulg(p))
        p = p * s % R
    return b"".join(out)


def lagrange_value(points, values, x):
    """the polynomial of degree < m through (points[t], values[t]), at x"""
    acc = 0
    for j, (pj, vj) in enumerate(zip(points, values)):
        num = den = 1
        for i, pi in enumerate(points):
            if i != j:
                num, den = num * (x - pi) % R, den * (pj - pi) % R
        acc = (acc + vj * num * inv(den)) % R
    return acc


def interpolate(points, values):
    """its coefficients, lowest first"""
    m = len(points)
    out = [0] * m
    for j in range(m):
        num, den = [1], 1
        for i in range(m):
            if i != j:
                nxt = [0] * (len(num) + 1)
                for t, c in enumerate(num):
                    nxt[t + 1] = (nxt[t + 1] + c) % R
                    nxt[t] = (nxt[t] - points[i] * c) % R
                num, den = nxt, den * (points[j] - points[i]) % R
        f = values[j] * inv(den) % R
        for t in range(m):
            out[t] = (out[t] + num[t] * f) % R
    return out


def sets_of(mos, queries):
    """the query sets in one shape for both schemes: {"shifts": [..], "polys": [..], "evals": [[per shift] per polynomial]}"""
    if mos == GWC19:
        return [{"shifts": [st["shift"]], "polys": st["polys"], "evals": [[e] for e in st["evals"]]} for st in K.gwc19_query_sets(queries)]
    return K.bdfg21_query_sets(queries)


def plan(mos, queries, z, c):
    """per set: polys, scalars c^j, points z shift_t, r (the coefficients of the interpolation of the c-combined evaluations)"""
    out = []
    for st in sets_of(mos, queries):
        pc = K.powers(c, len(st["polys"]))
        points = [z * sh % R for sh in st["shifts"]]
        vals = [sum(pc[j] * st["evals"][j][t] for j in range(len(pc))) % R for t in range(len(points))]
        out.append({"polys": list(st["polys"]), "scalars": pc, "points": points, "vals": vals, "r": interpolate(points, vals)})
    return out


def plan_finish(pl, gamma, z_prime):
    """Bdfg21 after z': L = sum scalars[j] polys[idx[j]] - z1 h - constant"""
    idx, scalars, constant, z1 = [], [], 0, None
    for i, st in enumerate(pl):
        zi = 1
        for p in st["points"]:
            zi = zi * (z_prime - p) % R
        if z1 is None:
            z1 = zi
        f = pow(gamma, i, R) * z1 * inv(zi) % R
        constant = (constant + f * horner(st["r"], z_prime)) % R
        idx += st["polys"]
        scalars += [f * sc % R for sc in st["scalars"]]
    return {"idx": idx, "scalars": scalars, "constant": constant, "z1": z1}


def gwc19_prove(s, polys, z, queries, v):
    """[W_k]: W_k = [(sum_i v^i p_i(s) - sum_i v^i e_i) / (s - z shift_k)] G"""
    ws = []
    for st in K.gwc19_query_sets(queries):
        pv = K.powers(v, len(st["polys"]))
        num = sum(pvi * (horner(polys[p], s) - e) for p, e, pvi in zip(st["polys"], st["evals"], pv)) % R
        ws.append(mulg(num * inv(s - z * st["shift"])))
    return ws


def bdfg21_h_at(s, polys, z, queries, mu, gamma):
    """h(s) = sum_i gamma^i (q_i(s) - r_i(s)) / Z_i(s), and per set (q_i(s), points, mu-combined evaluations)"""
    h, per_set = 0, []
    for i, st in enumerate(K.bdfg21_query_sets(queries)):
        pm = K.powers(mu, len(st["polys"]))
        points = [z * sh % R for sh in st["shifts"]]
        vals = [sum(pm[j] * st["evals"][j][t] for j in range(len(pm))) % R for t in range(len(points))]
        q_s = sum(pmj * horner(polys[p], s) for p, pmj in zip(st["polys"], pm)) % R
        z_s = 1
        for p in points:
            z_s = z_s * (s - p) % R
        h = (h + pow(gamma, i, R) * (q_s - lagrange_value(points, vals, s)) * inv(z_s)) % R
        per_set.append((q_s, points, vals))
    return h, per_set


def bdfg21_prove(s, polys, z, queries, mu, gamma, draw_z_prime):
    """(W, z', W'): W = [h(s)] G, z' = draw_z_prime(W), W' = [L(s) / (s - z')] G with
    L(s) = sum_i gamma^i (Z_1(z') / Z_i(z')) (q_i(s) - r_i(z')) - Z_1(z') h(s)"""
    h, per_set = bdfg21_h_at(s, polys, z, queries, mu, gamma)
    w = mulg(h)
    z_prime = draw_z_prime(w) % R
    big_l, z1 = 0, None
    for i, (q_s, points, vals) in enumerate(per_set):
        zi = 1
        for p in points:
            zi = zi * (z_prime - p) % R
        if z1 is None:
            z1 = zi
        big_l = (big_l + pow(gamma, i, R) * z1 * inv(zi) * (q_s - lagrange_value(points, vals, z_prime))) % R
    big_l = (big_l - z1 * h) % R
    return w, z_prime, mulg(big_l * inv(s - z_prime))


def commitments(s, polys):
    """[p(s)] G per polynomial, as points (None: the identity)"""
    return [O.g1_from_bytes(mulg(horner(p, s))) for p in polys]


def with_evals(polys, z, pairs):
    """[(poly, shift)] -> [(poly, shift, polys[poly](z shift))]"""
    return [(p, sh, horner(polys[p], z * sh % R)) for p, sh in pairs]


def standard_plonk_instance(rng, n, n_polys=17):
    """random polynomials of n coefficients in the query shape of oracle/kzg.py::standard_plonk_queries, with z"""
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_polys)]
    z = rng.randrange(1, R)
    return polys, z, with_evals(polys, z, K.standard_plonk_queries(rng, n_polys))


def draw_from(tag):
    """a deterministic stand-in for the transcript: z' from the bytes of W"""
    import hashlib

    return lambda w: int.from_bytes(hashlib.sha256(tag.encode() + bytes(w)).digest(), "little") % R


def set_shape_cases(rng):
    """name -> (polys, z, queries): the set shapes at which the provers take another path"""
    def rand_polys(count, n):
        return [[rng.randrange(R) for _ in range(n)] for _ in range(count)]

    cases = {}
    w1, w2 = rng.randrange(2, R), rng.randrange(2, R)
    polys, z = rand_polys(1, 5), rng.randrange(1, R)
    cases["one polynomial, one query"] = (polys, z, with_evals(polys, z, [(0, 1)]))
    polys, z = rand_polys(40, 64), rng.randrange(1, R)  # 40 terms: two passes of the linear combination
    cases["40 polynomials in one set"] = (polys, z, with_evals(polys, z, [(p, w1) for p in range(40)]))
    polys, z = rand_polys(3, 9), rng.randrange(1, R)
    cases["a pair given twice"] = (polys, z, with_evals(polys, z, [(0, 1), (1, 1), (1, w1), (0, 1), (2, w1), (1, w1)]))
    polys, z = rand_polys(2, 3), rng.randrange(1, R)  # as many points as coefficients: q - r = 0, the zero quotient
    three = [(0, 1), (0, w1), (0, w2)]
    cases["three points at n = 3, and a second set"] = (polys, z, with_evals(polys, z, three + [(1, w1)]))
    cases["three points at n = 3, alone"] = (polys[:1], z, with_evals(polys, z, three))
    polys, z = rand_polys(2, 1), rng.randrange(1, R)  # constants: every quotient is empty, every output the identity
    cases["constants, n = 1"] = (polys, z, with_evals(polys, z, [(0, 1), (1, w1)]))
    return cases
