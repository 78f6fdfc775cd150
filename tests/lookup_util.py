"""Shared helpers of the lookup tests: the sequential model over Python integers of include/snarkv_lookup.h -- the sort, halo2's
permute_expression_pair (the definition the device's parallel form is compared with, bit for bit) and the lookup product --
the reference's lookup constraints recomputed in integers, and the inputs that the CPU model test and the GPU test share."""
import os
import random
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as _BN  # noqa: E402
import pallas as _PA  # noqa: E402

FIELD = {"bn254": _BN.R, "pallas": _PA.R}


def pack(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def sort_model(vals, r):
    """what poly_sort_dev writes: the residues, ascending"""
    return sorted(v % r for v in vals)


def permute_model(A, S, u, r):
    """halo2's permute_expression_pair over the first u rows -> (A', S', [missing, distinct, 0, 0]).  Where halo2 returns an
    error (an input value the table lacks) the row keeps its input value and the count goes to the status."""
    A1 = sorted(v % r for v in A[:u])
    left = Counter(v % r for v in S[:u])
    S1, repeated, missing, distinct = [None] * u, [], 0, 0
    for i, v in enumerate(A1):
        if i == 0 or v != A1[i - 1]:
            distinct += 1
            S1[i] = v  # first occurrence: the table row is the input value
            if left[v] == 0:
                missing += 1  # halo2 returns an error here
            else:
                left[v] -= 1
        else:
            repeated.append(i)
    rest = [v for v in sorted(left) for _ in range(left[v])]  # ascending, with multiplicity
    for v in rest:  # halo2: repeated_input_rows.pop(), from the LAST repeated row down
        if repeated:
            S1[repeated.pop()] = v
    assert not repeated and None not in S1  # u table values, at most u - len(repeated) of them used
    return A1, S1, [missing, distinct, 0, 0]


def product_model(A, S, A1, S1, beta, gamma, start, r):
    """-> (z, total): z[0] = start, z[i+1] = z[i] (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)); a zero
    denominator gives the factor zero, as the batch inversion leaves it"""
    z, acc = [], start
    for a, s, a1, s1 in zip(A, S, A1, S1):
        z.append(acc)
        den = (a1 + beta) * (s1 + gamma) % r
        acc = acc * (a + beta) * (s + gamma) % r * (pow(den, -1, r) if den else 0) % r
    return z, acc


def constraints_hold(A, S, A1, S1, u, r):
    """the reference's lookup constraints on the permuted columns, in integers: A'[0] = S'[0], (A'[i] - S'[i])(A'[i] - A'[i-1])
    = 0 for 0 < i < u, and A', S' are rearrangements of A, S"""
    if u and (A1[0] - S1[0]) % r:
        return False
    for i in range(1, u):
        if (A1[i] - S1[i]) * (A1[i] - A1[i - 1]) % r:
            return False
    return Counter(v % r for v in A[:u]) == Counter(A1[:u]) and Counter(v % r for v in S[:u]) == Counter(S1[:u])


# ---------------------------------------------------------------- inputs

def sort_inputs(n, r, seed):
    """name -> n values below 2^256: what tests/test_gpu_lookup.py sorts at every length"""
    rnd = random.Random("lookup-sort-%s-%d" % (seed, n))
    uniform = [rnd.randrange(r) for _ in range(n)]
    base = sum(rnd.randrange(1 << 32) << (32 * w) for w in range(1, 7))  # words 0 and 7 clear, the rest random
    edge = [0, r - 1, r, r + 1, (1 << 256) - 1, 1, r - 2, 2 * r, 2 * r + 5]
    return {
        "uniform": uniform,
        "all equal": [uniform[0]] * n,
        "sorted": sorted(uniform),
        "reversed": sorted(uniform, reverse=True),
        "small": [rnd.randrange(16) for _ in range(n)],
        "word 0": [base | rnd.randrange(1 << 32) for _ in range(n)],
        "word 7": [base | (rnd.randrange(1 << 28) << 224) for _ in range(n)],
        "edges": [edge[rnd.randrange(len(edge))] if rnd.randrange(2) else rnd.randrange(r) for _ in range(n)],
    }


def permute_cases(u, r, tile, block, seed):
    """name -> (A, S, missing): the cases of the issue at u rows, as far as u has room; `missing` is the number of distinct
    input values that the table lacks"""
    rnd = random.Random("lookup-permute-%s-%d" % (seed, u))
    cases = {}
    S = [rnd.randrange(r) for _ in range(u)]
    A = list(S)
    rnd.shuffle(A)
    cases["shuffle"] = (A, S, 0)
    c = rnd.randrange(r)
    cases["constant input"] = ([c] * u, [c] + [rnd.randrange(r) for _ in range(u - 1)], 0)
    if u >= 256:
        table = [rnd.randrange(r) for _ in range(256)]
        S = (table * (u // 256 + 1))[:u]
        rnd.shuffle(S)
        cases["range table"] = ([rnd.choice(table) for _ in range(u)], S, 0)
    if u >= 64:
        # table values held 1, 2 and 5 times; each used fewer times, as many times and more times than held; values unused
        held = {}
        for h in (1, 2, 5):
            for use in (max(h - 1, 1), h, h + 3):
                held[rnd.randrange(r)] = (h, use)
        A = [v for v, (h, use) in held.items() for _ in range(use)]
        S = [v for v, (h, use) in held.items() for _ in range(h)]
        filler = rnd.choice(list(held))
        A += [filler] * (u - len(A))
        S += [rnd.randrange(r) for _ in range(u - len(S))]  # table values no input uses
        rnd.shuffle(A)
        rnd.shuffle(S)
        cases["multiplicities"] = (A, S, 0)
    # a run of equal input values across the border of a sort tile and of a scan block: small distinct values in front of it
    # place it exactly, larger ones follow; seven rows long, or as many as u has behind the border
    for name, border in (("run over tile border", tile), ("run over scan border", block)):
        if u > border:
            lo = max(border - 3, 1)
            run_len = min(7, u - lo)
            assert lo < border < lo + run_len
            small = list(range(1, lo + 1))
            v = lo + 10
            big = [v + 1 + i for i in range(u - lo - run_len)]
            A = small + [v] * run_len + big
            S = small + [v] + big + [rnd.randrange(1 << 200, r) for _ in range(run_len - 1)]
            assert len(A) == len(S) == u and sorted(A)[lo:lo + run_len] == [v] * run_len
            rnd.shuffle(A)
            rnd.shuffle(S)
            cases[name] = (A, S, 0)
    for m in (1, 7):
        if u >= 4 * m + 4:
            table = [rnd.randrange(r) for _ in range(u // 2)]
            S = table + [rnd.choice(table) for _ in range(u - len(table))]
            absent = [rnd.randrange(r) for _ in range(m)]
            A = [rnd.choice(table) for _ in range(u - 2 * m)] + absent + absent  # each missing value twice: first and repeated
            rnd.shuffle(A)
            rnd.shuffle(S)
            cases["%d missing" % m] = (A, S, m)
    return cases
