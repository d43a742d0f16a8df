"""CPU check of the two-strand outside recursion (desirna_amd/csrc/fold_cofold_outside.hpp), compiled unmodified together with
cofold_pf_kernel against the HIP stand-in of tests/emu/ into a library of its own.  The reference pins no pair probability or
ensemble defect for two strands, so the values are checked against explicit enumeration of every co-fold structure (weights
from the oracle's two-strand evaluation) and against identities that follow from the definition."""
import numpy as np
import pytest

from tests.emu.emu import cofold_edef, cofold_edef_many
from tests.test_cofold_subopt_emulated import _enumeration_cases, _rand, cofold_structures

KT = 1.98717e-3 * 310.15
EDEF_TOL = 1e-10
PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}


def homodimer_cases():
    rng = np.random.default_rng(7)
    out = []
    for k in range(12):
        n = int(rng.integers(4, 8))
        x = "".join(rng.choice(list(("ACGU", "GC", "AUUAGC")[k % 3]), n))
        out.append(x + "&" + x)
    return out


def pairs_of(db):
    stk, out = [], []
    for k, ch in enumerate(db, 1):
        if ch == "(":
            stk.append(k)
        elif ch == ")":
            out.append((stk.pop(), k))
    return out


def defect_from_matrix(P, target):
    """the definition: (1/L) [ sum_{i unpaired} sum_j P(i,j) + sum_{i paired with m} (1 - P(i,m)) ], P upper triangular, 1-based"""
    target = target.replace("&", "")
    n = len(target)
    S = P + P.T
    partner = {}
    for i, j in pairs_of(target):
        partner[i], partner[j] = j, i
    tot = 0.0
    for i in range(1, n + 1):
        tot += 1.0 - S[i, partner[i]] if i in partner else S[i, 1:].sum()
    return tot / n


def enumerate_ensemble(oracle, s):
    """(P, F, structures): pair probabilities and free energy by enumeration, weight = exp(-E / kT) with the oracle's two-strand
    energy (DuplexInit included for connected structures), connected weights halved when the strands are equal"""
    a, b = s.split("&")
    cut, flat = len(a), a + b
    n = len(flat)
    dbs = cofold_structures(flat, cut)
    P, Z = np.zeros((n + 1, n + 1)), 0.0
    for db in dbs:
        w = np.exp(-oracle.eval_structure(flat, db, cut) / 100.0 / KT)
        prs = pairs_of(db)
        if a == b and any(i <= cut < j for i, j in prs):
            w *= 0.5
        Z += w
        for i, j in prs:
            P[i, j] += w
    return P / Z, -KT * np.log(Z), dbs


@pytest.mark.parametrize("nt", [64, 128])
@pytest.mark.parametrize("kind", ["hetero", "homo"])
def test_probabilities_against_enumeration(oracle, nt, kind):
    """A case enters if the integer evaluation and the partition function's loop model agree on its free energy to 1e-6 kcal/mol
    (the oracle alone: 47 of the 60 pairs, 11 of the 12 homodimers); then |dP| and |dEdef| < 1e-5: a free-energy mismatch of
    1e-6 is a relative weight error of 1e-6 / kT = 1.6e-6, times a margin of about 6."""
    cases, need = (_enumeration_cases(), 40) if kind == "hetero" else (homodimer_cases(), 9)
    assert len(cases) == (60 if kind == "hetero" else 12)
    rng = np.random.default_rng(11)
    ref, targets = [], []
    for s in cases:
        P, F, dbs = enumerate_ensemble(oracle, s)
        ref.append((P, F))
        targets.append(dbs[int(rng.integers(len(dbs)))])
    got = cofold_edef_many(cases, targets, nt=nt)
    entered = 0
    for s, tg, (P, F), (ed, bpp, F4, st) in zip(cases, targets, ref, got):
        assert st == 0, s
        if abs(F - oracle.cofold_pf(s)[3]) >= 1e-6:
            continue
        entered += 1
        dP, dE = np.abs(bpp - P).max(), abs(ed - defect_from_matrix(P, tg))
        print(s, tg, "max|dP| %.3e |dEdef| %.3e" % (dP, dE))
        assert dP < 1e-5, (s, nt)
        assert dE < 1e-5, (s, tg, nt)
    assert entered >= need, entered


def test_strands_that_cannot_pair(oracle):
    """nothing joins {G, C} to A: P inside the foldable strand is the one-strand matrix (the part of the outside weights that
    must not get kappa), every other entry is 0"""
    rng = np.random.default_rng(5)
    strands = [_rand(rng, la, "GC") for la in (9, 11, 13, 14)]
    cases = [x + "&" + "A" * lb for x, lb in zip(strands, (6, 4, 9, 12))]
    cases += ["A" * lb + "&" + x for x, lb in zip(strands, (5, 8, 4, 10))]       # mirrored
    targets = ["." * (len(s) - 1) for s in cases]
    for s, (ed, bpp, F4, st) in zip(cases, cofold_edef_many(cases, targets)):
        assert st == 0, s
        a, b = s.split("&")
        x, off = (a, 0) if a[0] != "A" else (b, len(a))
        ed1, P1 = oracle.ensemble_defect(x, "." * len(x), want_bpp=True)
        want = np.zeros_like(bpp)
        want[off + 1:off + len(x) + 1, off + 1:off + len(x) + 1] = P1[1:, 1:]
        assert np.abs(bpp - want).max() < EDEF_TOL, s
        assert abs(ed * (len(s) - 1) - ed1 * len(x)) < EDEF_TOL * len(s), s


def test_identities_random(oracle):
    """row sums, structural zeros, and Edef against the all-dots target = (1/L) sum_i sum_j P(i,j)"""
    rng = np.random.default_rng(33)
    cases = [_rand(rng, la, alpha) + "&" + _rand(rng, lb, alpha)
             for la, lb, alpha in ((12, 9, "ACGU"), (10, 10, "ACGU"), (13, 11, "GGCCAU"), (5, 17, "ACGU")) for _ in range(3)]
    for s, (ed, bpp, F4, st) in zip(cases, cofold_edef_many(cases, ["." * (len(s) - 1) for s in cases])):
        assert st == 0, s
        cut, flat = s.index("&"), s.replace("&", "")
        n = len(flat)
        assert abs(F4[3] - oracle.cofold_pf(s)[3]) < 1e-9, s
        assert bpp.min() >= 0.0 and bpp.max() <= 1.0
        S = bpp + bpp.T
        assert S.sum(1).max() <= 1.0 + 1e-12, s
        assert abs(ed - S[1:, 1:].sum() / n) < EDEF_TOL, s
        assert bpp[0].max() == 0.0 and bpp[:, 0].max() == 0.0
        for i in range(1, n + 1):
            for j in range(1, n + 1):
                joins = i <= cut < j
                if j <= i or flat[i - 1] + flat[j - 1] not in PAIRS or (not joins and j - i < 4):
                    assert bpp[i, j] == 0.0, (s, i, j)


def test_homodimer_rotation():
    """X&X: the structure set is closed under rotation by cut and the weights are equal"""
    rng = np.random.default_rng(17)
    xs = [_rand(rng, int(rng.integers(8, 13)), "GGCCAU") for _ in range(6)]
    cases = [x + "&" + x for x in xs]
    for x, (ed, bpp, F4, st) in zip(xs, cofold_edef_many(cases, ["." * (2 * len(x)) for x in xs])):
        assert st == 0, x
        cut = len(x)
        assert bpp.max() > 1e-3
        for i in range(1, cut + 1):
            for j in range(i + 1, 2 * cut + 1):
                if j <= cut:
                    assert abs(bpp[i, j] - bpp[i + cut, j + cut]) < EDEF_TOL, (x, i, j)
                elif j - cut != i:
                    a, b = sorted((j - cut, i + cut))
                    assert abs(bpp[i, j] - bpp[a, b]) < EDEF_TOL, (x, i, j)


def test_batch_and_bad_letter():
    """several pairs through one workspace slot one after the other give the single-pair bits (nothing of a previous pair is
    read); a bad letter is ST_BAD_CHAR with a defect of 0"""
    seqs = ["GGGAAC&GUUCCC", "GCGCAU&AUGCGC", "GGGXAC&GUUCCC", "GGGAAC&GUUCCC"]
    tg = "((((..&..))))"
    ed, bpp, F4, st = cofold_edef(seqs, tg, nt=64)
    assert list(st) == [0, 0, 1, 0] and ed[2] == 0.0
    assert ed[0] == ed[3] and (bpp[0] == bpp[3]).all()
    for k, (e1, b1, f1, s1) in enumerate(cofold_edef_many(seqs[:2], [tg, tg], nt=64)):
        assert s1 == 0 and e1 == ed[k] and (b1 == bpp[k]).all()
    assert abs(ed[0] - defect_from_matrix(bpp[0], tg)) < 1e-12
