"""Reference of the stochastic traceback's tests (tests/test_sampling_emulated.py, tests/test_sampling_gpu.py): exact structure
probabilities from the oracle's structure walk, a plain enumerator of all structures of a short sequence, and the rule by which a
sample frequency is held to a probability.  A plain helper module (no fixtures, no pytest configuration); it looks at the oracle
alone, never at the code under test.

    p(s) = oracle.boltzmann_weight(seq, s) / exp(-oracle.pf(seq) / kT)

boltzmann_weight walks the loops of ONE structure -- it shares nothing with the inside fill whose tables the sampler reads."""
import math
from collections import Counter

import numpy as np

from tests.pair_prob_ref import PAIRS, pairs_of

KT = 1.98717e-3 * 310.15          # kcal/mol at 37 C, as the pair-probability reference takes it (tests/test_pair_prob_reference.py)
TURN = 3


def enumerate_structures(seq):
    """every secondary structure of seq as dot-bracket: canonical pairs, at least three bases enclosed, nested"""
    n = len(seq)
    can = [[seq[i] + seq[j] in PAIRS and j - i > TURN for j in range(n)] for i in range(n)]
    memo = {}

    def rec(i, j):                  # structures of seq[i..j]
        if j - i < TURN + 1:
            return ["." * max(0, j - i + 1)]
        if (i, j) in memo:
            return memo[i, j]
        out = ["." + s for s in rec(i + 1, j)]
        for k in range(i + TURN + 1, j + 1):
            if can[i][k]:
                ins, rest = rec(i + 1, k - 1), rec(k + 1, j)
                out += ["(" + a + ")" + b for a in ins for b in rest]
        memo[i, j] = out
        return out

    return rec(0, n - 1)


def structure_probability(oracle, seq, db):
    return oracle.boltzmann_weight(seq, db) / math.exp(-oracle.pf(seq) / KT)


def exact_distribution(oracle, seq):
    """{structure: p} over the whole enumeration; the probabilities sum to 1 up to the oracle's rounding"""
    Z = math.exp(-oracle.pf(seq) / KT)
    return {db: oracle.boltzmann_weight(seq, db) / Z for db in enumerate_structures(seq)}


def bound(p, S):
    """six standard deviations of a frequency from S draws, the variance floored at 10 expected counts"""
    return 6.0 * math.sqrt(max(p * (1.0 - p), 10.0 / S) / S)


def meets(f, p, S):
    return abs(f - p) <= bound(p, S)


def check_distribution(samples, dist, p_min=1e-3):
    """samples: the S sampled strings of one sequence; dist: exact_distribution.  Returns the list of failures (empty = pass):
    every sample must be a member of the enumeration, every structure with p >= p_min and the bucket of all others must meet the
    rule."""
    S = len(samples)
    cnt = Counter(samples)
    bad = ["not in the enumeration: %r" % s for s in cnt if s not in dist]
    big = [s for s, p in dist.items() if p >= p_min]
    for s in big:
        if not meets(cnt.get(s, 0) / S, dist[s], S):
            bad.append("%s: f = %.5f, p = %.5f, bound %.5f" % (s, cnt.get(s, 0) / S, dist[s], bound(dist[s], S)))
    p_other = 1.0 - sum(dist[s] for s in big)
    f_other = sum(c for s, c in cnt.items() if s not in big) / S
    if not meets(f_other, p_other, S):
        bad.append("others: f = %.5f, p = %.5f, bound %.5f" % (f_other, p_other, bound(p_other, S)))
    return bad


def pair_frequencies(samples, n):
    """(n+1, n+1) upper-triangular, 1-based: fraction of the samples that hold the pair (i,j)"""
    F = np.zeros((n + 1, n + 1))
    for s, c in Counter(samples).items():
        for i, j in pairs_of(s):
            F[i, j] += c
    return F / len(samples)


def check_pair_frequencies(samples, P, pairs):
    """failures of the rule over `pairs` (the entries the reference matrix fills); P as pair_prob_ref.reference_matrix gives it"""
    S, n = len(samples), len(samples[0])
    F = pair_frequencies(samples, n)
    return ["(%d,%d): f = %.5f, p = %.5f, bound %.5f" % (i, j, F[i, j], P[i, j], bound(P[i, j], S))
            for i, j in pairs if not meets(F[i, j], min(max(P[i, j], 0.0), 1.0), S)]


def well_formed(seq, db):
    """balanced, canonical pairs, at least three bases enclosed by each pair, only ( ) ."""
    if len(db) != len(seq) or set(db) - set("()."):
        return False
    stk = []
    for k, ch in enumerate(db):
        if ch == "(":
            stk.append(k)
        elif ch == ")":
            if not stk:
                return False
            o = stk.pop()
            if seq[o] + seq[k] not in PAIRS or k - o <= TURN:
                return False
    return not stk


def has_multiloop(db):
    """some pair closes a loop with at least two inner stems"""
    stk = []
    for ch in db:
        if ch == "(":
            stk.append(0)
        elif ch == ")":
            if stk.pop() >= 2:
                return True
            if stk:
                stk[-1] += 1
    return False
