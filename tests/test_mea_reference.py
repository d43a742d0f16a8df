"""The yardstick of the MEA tests pinned (tests/mea_ref.py, CPU): on the oracle's pair probabilities of short sequences the numpy
recurrence must reach the exhaustive maximum of the expected accuracy over every structure, its traceback must be a structure of
that value, and the centroid's distance must be the expected base-pair distance."""
import numpy as np
import pytest

from tests import mea_ref as mr
from tests import pair_prob_ref as ppr
from tests import sampling_ref as sr

GAMMAS = (0.25, 1.0, 4.0)
SEQS = ["GGGAAAUCC", "GCGCAAAAGCGC", "GGUGUUAGCUCAU", "ACGUACGUACGUAC", "GGGAAACCCAAAGG", "GCCAAGGAAACCGC", "AAAAAAAAAA", "GAAAC"]
SEQS += [ppr.rand_seq(np.random.default_rng(50 + k), 10 + k % 5, ("ACGU", "GC", "GGCCAU")[k % 3]) for k in range(10)]


@pytest.mark.parametrize("seq", SEQS)
def test_recurrence_reaches_the_exhaustive_maximum(oracle, seq):
    n = len(seq)
    assert n <= 14
    _, P = oracle.ensemble_defect(seq, "." * n, want_bpp=True)
    structures = sr.enumerate_structures(seq)
    for g in GAMMAS:
        db, val = mr.mea(P, g)
        want = mr.exhaustive_max(P, structures, g)
        assert abs(val - want) <= mr.tol(n, g), (seq, g, val, want)
        assert db in structures and mr.well_formed(P, db)
        assert abs(mr.expected_accuracy(P, db, g) - val) <= mr.tol(n, g)


def test_tie_rule_on_exact_matrices():
    # two pairs of column 4 with the same probability: q = (3/4, 3/4, 1, 1/2)
    P = np.zeros((5, 5))
    P[1, 4] = P[2, 4] = 0.25
    q = mr.unpaired_probs(P)
    assert list(q[1:]) == [0.75, 0.75, 1.0, 0.5]
    db, val = mr.mea(P, 2.0)                  # pair: 2 gamma P = 1, both ends unpaired: 1.25 -> nothing pairs
    assert db == "...." and val == 3.0
    db, val = mr.mea(P, 2.5)                  # 1.25 against 1.25: a tie, "j unpaired" first
    assert db == "...." and val == 3.0
    db, val = mr.mea(P, 4.0)                  # 2 against 1.25 for either pair; equal values, k ascending: (1,4)
    assert db == "(..)" and val == 0.75 + 1.0 + 2.0


def test_centroid_distance_is_the_expected_distance(oracle):
    seq = "GCGCAAAAGCGC"
    _, P = oracle.ensemble_defect(seq, "." * len(seq), want_bpp=True)
    cen, d = mr.centroid(P)
    dist = sr.exact_distribution(oracle, seq)
    cp = set(ppr.pairs_of(cen))
    want = sum(p * len(cp ^ set(ppr.pairs_of(s))) for s, p in dist.items())
    assert cen == "((((....))))" and abs(d - want) < 1e-9
    assert mr.centroid(np.zeros((6, 6))) == (".....", 0.0)
