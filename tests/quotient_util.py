"""Shared helpers of the quotient tests: the reference over Python integers of include/snarkv_quotient.h -- the gate program
interpreted row by row, the values on the extended coset, the division by the vanishing polynomial and the way back to
coefficients (the transforms are tests/ntt_util.py's) -- and the small circuit that the CPU model test states on integers and
the GPU test runs end to end."""
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ntt_util as U  # noqa: E402

FIELD = {c: m.R for c, m in U.CURVES.items()}
GENERATOR = {"bn254": (7, 28), "pallas": (5, 32)}  # g and S of include/snarkv_ntt.h
ADD, SUB, MUL, FMA = 0, 1, 2, 3
REGS = 16
pack, unpack, horner = U.pack, U.unpack, U.horner


def zeta(curve):
    """halo2's ZETA, a primitive cube root of unity: the coset shift of the extended domain"""
    r, (g, _) = FIELD[curve], GENERATOR[curve]
    z = pow(g, (r - 1) // 3, r)
    assert z != 1 and pow(z, 3, r) == 1
    return z


def decode(code):
    """packed snarkv_quot_instr -> [(op, dst, a, b, c)]"""
    out = []
    for at in range(0, len(code), 16):
        op, dst, zero, a, b, c = struct.unpack_from("<BBHIII", code, at)
        assert zero == 0
        out.append((op, dst, a, b, c))
    return out


def row_of(i, rot, e, n_ext):
    """halo2's get_rotation_idx with rot_scale = 2^e: Python's % is the euclidean remainder"""
    return (i + rot * (1 << e)) % n_ext


def interpret(curve, cols, k, e, instrs, consts):
    """what snarkv_quotient_eval_dev computes: cols = lists of 2^(k+e) integers (any below 2^256), instrs as decode() gives
    them -> the 2^(k+e) canonical values of the last destination"""
    r, n_ext = FIELD[curve], 1 << (k + e)
    out = []
    for i in range(n_ext):
        regs = [None] * REGS

        def operand(w):
            kind = w >> 30
            if kind == 0:
                return regs[w & 0x3FFFFFFF]
            if kind == 1:
                return consts[w & 0x3FFFFFFF]
            assert kind == 2
            rot = (w >> 20) & 0x3FF
            rot -= 1024 if rot >= 512 else 0
            return cols[w & 0xFFFFF][row_of(i, rot, e, n_ext)]

        for op, dst, a, b, c in instrs:
            x, y = operand(a), operand(b)
            regs[dst] = (x + y if op == ADD else x - y if op == SUB else x * y if op == MUL else x * y + operand(c)) % r
        out.append(regs[instrs[-1][1]])
    return out


def extend(curve, coeffs, k, e, shift):
    """out[i] = f(shift W^i) over the 2^(k+e) domain: halo2's coeff_to_extended"""
    assert len(coeffs) == 1 << k
    return U.reference(curve, list(coeffs) + [0] * ((1 << (k + e)) - (1 << k)), U.FORWARD, shift)


def vanishing_table(curve, k, e, shift):
    """(shift W^j)^n - 1 for j < 2^e: the values the divisor takes, at row i the entry i mod 2^e"""
    r = FIELD[curve]
    wn = U.omega(curve, e)  # W^n generates the 2^e domain
    assert wn == pow(U.omega(curve, k + e), 1 << k, r)
    sn = pow(shift, 1 << k, r)
    return [(sn * pow(wn, j, r) - 1) % r for j in range(1 << e)]


def div_vanishing(curve, vals, k, e, shift):
    r = FIELD[curve]
    inv = [pow(t, -1, r) if t else 0 for t in vanishing_table(curve, k, e, shift)]
    return [v * inv[i % (1 << e)] % r for i, v in enumerate(vals)]


def to_coeffs(curve, vals, shift_inv):
    """the inverse transform with the shift s^-1: values on the coset back to coefficients"""
    return U.reference(curve, list(vals), U.INVERSE, shift_inv)


def quotient(curve, coeff_cols, k, e, instrs, consts, shift):
    """what snarkv_quotient_dev computes -> the 2^(k+e) coefficients of h"""
    r = FIELD[curve]
    ext = [extend(curve, c, k, e, shift) for c in coeff_cols]
    h = div_vanishing(curve, interpret(curve, ext, k, e, instrs, consts), k, e, shift)
    return to_coeffs(curve, h, pow(shift, -1, r))


ROTATIONS = [-512, -1, 0, 1, 511]


def random_program(Q, rnd, n_instr, n_cols, n_consts):
    """a valid program of n_instr instructions over all four ops -> [(op, dst, a, b, c)].  Destinations walk the 16 registers
    first (so a program of 22 or more uses them all), every fourth instruction overwrites one of its own sources, and the
    rotations come from ROTATIONS."""
    written, out = [], []

    def operand(must_be=None):
        if must_be is not None:
            return Q.REG(must_be)
        kind = rnd.randrange(3 if written else 2)
        if kind == 0:
            return Q.COL(rnd.randrange(n_cols), rnd.choice(ROTATIONS))
        if kind == 1:
            return Q.CONST(rnd.randrange(n_consts))
        return Q.REG(rnd.choice(written))

    for pc in range(n_instr):
        op = rnd.choice([ADD, SUB, MUL, FMA])
        own = rnd.choice(written) if written and pc % 4 == 3 else None
        dst = own if own is not None else len(written) if len(written) < REGS else rnd.randrange(REGS)
        ops = [operand(own), operand()]
        if rnd.randrange(2):
            ops.reverse()
        ops.append(operand() if op == FMA else 0)
        out.append((op, dst, ops[0], ops[1], ops[2]))
        if dst not in written:
            written.append(dst)
    return out


def pack_program(Q, instrs):
    return b"".join(Q.pack_instr(*i) for i in instrs)


# ---------------------------------------------------------------- the small circuit
# Three witness columns a, b, c over n = 2^k rows: the gate q_mul (a b - c) + q_add (a + b - c), the copy constraints
# c[i] = a[i + 1], the permutation argument over the three columns (full cycle, no blinding rows: the total is one).
# Columns of the program: 0 a, 1 b, 2 c, 3 q_mul, 4 q_add, 5 Z, 6 l_0, 7..9 sigma_j, 10 X.
COLS = 11
COL_A, COL_B, COL_C, COL_QM, COL_QA, COL_Z, COL_L0, COL_S0, COL_X = 0, 1, 2, 3, 4, 5, 6, 7, 10


class Circuit:
    def __init__(self, curve, k, bad=None, seed="quotient-circuit"):
        r, (g, _) = FIELD[curve], GENERATOR[curve]
        n = 1 << k
        rnd = random.Random("%s-%s-%d" % (seed, curve, k))
        self.curve, self.k, self.n, self.r = curve, k, n, r
        self.w, self.delta = U.omega(curve, k), g
        a, b, c = [0] * n, [rnd.randrange(r) for _ in range(n)], [0] * n
        qm = [rnd.randrange(2) for _ in range(n)]
        qm[0], qm[1] = 1, 0  # both gates are used
        qa = [1 - q for q in qm]
        a[0] = rnd.randrange(r)
        for i in range(n):
            c[i] = (a[i] * b[i] if qm[i] else a[i] + b[i]) % r
            if i + 1 < n:
                a[i + 1] = c[i]
        if bad == "gate":  # one cell of c changed, the copy of it kept
            c[5] = (c[5] + 1) % r
            a[6] = c[5]
        if bad == "copy":  # the constraint c[6] = a[7] broken, the gates kept
            a[7] = (a[7] + 1) % r
            c[7] = (a[7] * b[7] if qm[7] else a[7] + b[7]) % r
            a[8] = c[7]
        self.ids = [[pow(self.delta, j, r) * pow(self.w, i, r) % r for i in range(n)] for j in range(3)]
        self.sigma = [list(x) for x in self.ids]
        for i in range(n - 1):  # the cycle (c, i) <-> (a, i + 1)
            self.sigma[2][i], self.sigma[0][i + 1] = self.ids[0][i + 1], self.ids[2][i]
        self.a, self.b, self.c, self.qm, self.qa = a, b, c, qm, qa
        self.beta, self.gamma, self.y = (rnd.randrange(1, r) for _ in range(3))
        self.l0 = [1] + [0] * (n - 1)

    def z(self):
        """-> (Z, total) on integers"""
        r, z = self.r, [1]
        for i in range(self.n):
            num = den = 1
            for j, v in enumerate((self.a, self.b, self.c)):
                num = num * (v[i] + self.beta * self.ids[j][i] + self.gamma) % r
                den = den * (v[i] + self.beta * self.sigma[j][i] + self.gamma) % r
            z.append(z[-1] * num % r * pow(den, -1, r) % r)
        return z[:-1], z[-1]

    def value_columns(self, z):
        """the columns of the program but X, as values on the 2^k domain"""
        return [self.a, self.b, self.c, self.qm, self.qa, z, self.l0] + self.sigma

    def coeff_columns(self, z):
        """all COLS columns as coefficients; the last is the polynomial X"""
        cols = [U.reference(self.curve, v, U.INVERSE) for v in self.value_columns(z)]
        return cols + [([0, 1] + [0] * (self.n - 2)) if self.n > 1 else [0]]

    def program(self, Q, permutation=True):
        """the program over the module Q = snark_verifier_amd.quotient: gate, l_0 (1 - Z) and the permutation product folded
        with y; the gate alone without `permutation`"""
        r, p = self.r, Q.Program()
        col = Q.COL
        p.mul(0, col(COL_A), col(COL_B))
        p.sub(0, Q.REG(0), col(COL_C))
        p.mul(0, Q.REG(0), col(COL_QM))
        p.add(1, col(COL_A), col(COL_B))
        p.sub(1, Q.REG(1), col(COL_C))
        p.fma(0, col(COL_QA), Q.REG(1), Q.REG(0))  # the gate
        if not permutation:
            return p
        beta, gamma, y = p.const(self.beta), p.const(self.gamma), p.const(self.y)
        p.sub(1, p.const(1), col(COL_Z))
        p.mul(1, Q.REG(1), col(COL_L0))
        p.fma(0, Q.REG(0), y, Q.REG(1))  # gate y + l_0 (1 - Z)
        for j in range(3):  # r2 = Z(wX) prod (v + beta sigma + gamma)
            p.fma(3, beta, col(COL_S0 + j), col(COL_A + j))
            p.add(3, Q.REG(3), gamma)
            if j == 0:
                p.mul(2, Q.REG(3), col(COL_Z, 1))
            else:
                p.mul(2, Q.REG(2), Q.REG(3))
        for j in range(3):  # r4 = Z(X) prod (v + beta delta^j X + gamma)
            p.fma(5, p.const(self.beta * pow(self.delta, j, r) % r), col(COL_X), col(COL_A + j))
            p.add(5, Q.REG(5), gamma)
            if j == 0:
                p.mul(4, Q.REG(5), col(COL_Z))
            else:
                p.mul(4, Q.REG(4), Q.REG(5))
        p.sub(2, Q.REG(2), Q.REG(4))
        p.fma(0, Q.REG(0), y, Q.REG(2))
        return p

    def expression(self, coeffs, x, permutation=True):
        """the same expression at a point x, from the columns' coefficients (Z at w x as well)"""
        r = self.r
        return self.expression_of(x, [horner(c, x, r) for c in coeffs[:10]], horner(coeffs[COL_Z], x * self.w % r, r), permutation)

    def expression_of(self, x, values, z_next, permutation=True):
        """... from the values of the first ten columns at x and of Z at w x"""
        r = self.r
        A, B, C, QM, QA, Z, L0, S0, S1, S2 = values
        gate = (QM * (A * B - C) + QA * (A + B - C)) % r
        if not permutation:
            return gate
        left, right = z_next, Z
        for j, (v, s) in enumerate(((A, S0), (B, S1), (C, S2))):
            left = left * (v + self.beta * s + self.gamma) % r
            right = right * (v + self.beta * pow(self.delta, j, r) * x + self.gamma) % r
        return ((gate * self.y + L0 * (1 - Z)) * self.y + left - right) % r


def identity_holds(circuit, coeffs, h, x, permutation=True):
    """h(x) (x^n - 1) == expr(x)"""
    r = circuit.r
    return horner(h, x, r) * (pow(x, circuit.n, r) - 1) % r == circuit.expression(coeffs, x, permutation)
