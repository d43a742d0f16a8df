"""Free energies with positions held unpaired, by ENUMERATION: the reference of tests/test_access_*.py.  A plain helper module
(no fixtures, no pytest configuration).

    F[mask] = -kT ln  sum  w(s)     over the structures s that leave every masked position unpaired,

w = oracle.boltzmann_weight, the partition function's loop model applied to one structure.  The structure set is the fill's:
canonical pairs only, at least 3 nucleotides enclosed by a pair, and a pair that directly encloses exactly one pair has at most
MAXLOOP unpaired nucleotides between them.  Every case is checked by len(structures) == oracle.count_structures(seq), and the
enumeration is held to oracle.pf_forbid(seq, i, 0) -- the pinned fill with every pair of i forbidden -- at every position
(tests/test_access_reference.py).  A masked nucleotide keeps its letter in every energy term: the weight of a structure does
not depend on the mask, only whether it counts.

Everything here looks at the oracle alone, never at the code under test."""
import functools

import numpy as np

from oracle.pyoracle import KT
from tests import kbest_ref, pair_prob_ref

MAXLOOP = 30
CAP = 200_000                       # structures per enumerated case
MIN_EOPEN = 0.1                     # kcal/mol: a case needs a tested mask that costs at least this much
SEED = 20261

# stems that sit directly against their loops and ends: where an energy table indexed by the pairing code 4 would show
TIGHT = ("GGGAAACGGAAACCGA", "GGACGAAAGCAAAACC")


def structures(seq):
    """every structure of the fill's set, as a tuple of 0-based pairs (i, j)"""
    n = len(seq)
    partners = [[j for j in range(i + 4, n) if seq[i] + seq[j] in pair_prob_ref.PAIRS] for i in range(n)]

    @functools.lru_cache(maxsize=None)
    def S(i, j):
        """structures on [i, j]: (pairs, number of pairs not enclosed by another (2 = two or more), the first of them)"""
        while i <= j and not (partners[i] and partners[i][0] <= j):
            i += 1
        if i > j:
            return (((), 0, None),)
        out = list(S(i + 1, j))
        for k in partners[i]:
            if k > j:
                break
            inner = [a for a in S(i + 1, k - 1) if a[1] != 1 or (a[2][0] - i - 1) + (k - a[2][1] - 1) <= MAXLOOP]
            rest = S(k + 1, j)
            for a in inner:
                for b in rest:
                    out.append((((i, k),) + a[0] + b[0], min(2, 1 + b[1]), (i, k)))
        return tuple(out)

    return [s[0] for s in S(0, n - 1)]


def dot_bracket(n, pairs):
    db = ["."] * n
    for i, j in pairs:
        db[i], db[j] = "(", ")"
    return "".join(db)


class Ensemble:
    """the enumerated ensemble of one sequence: weights and which positions each structure pairs"""

    def __init__(self, oracle, seq):
        self.seq, self.n = seq, len(seq)
        ss = structures(seq)
        self.count = len(ss)
        if self.count > CAP:
            raise ValueError("%d structures: above the cap of %d" % (self.count, CAP))
        if self.count != oracle.count_structures(seq):
            raise ValueError("enumerated %d structures, the oracle counts %d" % (self.count, oracle.count_structures(seq)))
        self.w = np.array([oracle.boltzmann_weight(seq, dot_bracket(self.n, p)) for p in ss])
        self.paired = np.zeros((self.count, self.n), dtype=np.float32)
        for k, p in enumerate(ss):
            for i, j in p:
                self.paired[k, i] = self.paired[k, j] = 1.0
        self.F0 = -KT * np.log(self.w.sum())

    def free_energy(self, masks):
        """masks: (M, n) array, non-zero = stays unpaired -> float64[M] of F[mask] in kcal/mol"""
        m = (np.atleast_2d(np.asarray(masks)) != 0).astype(np.float32)
        keep = (self.paired @ m.T) == 0                    # (count, M): the structure pairs no masked position
        return np.array([-KT * np.log(self.w[keep[:, k]].sum()) for k in range(m.shape[0])])

    def opening_energy(self, masks):
        return self.free_energy(masks) - self.F0


# ------------------------------------------------------------------------------------------------ masks

def mask_rows(n, position_sets):
    """(M, n) uint8 from M collections of 1-based positions"""
    m = np.zeros((len(position_sets), n), dtype=np.uint8)
    for k, ps in enumerate(position_sets):
        for p in ps:
            m[k, p - 1] = 1
    return m


def single_masks(n):
    return mask_rows(n, [[i] for i in range(1, n + 1)])


def window_masks(n, W, every=1):
    return mask_rows(n, [range(a, a + W) for a in range(1, n - W + 2, every)])


def random_masks(n, count, seed):
    rng = np.random.default_rng([SEED, 7, seed, n])
    return (rng.random((count, n)) < rng.uniform(0.1, 0.5, size=(count, 1))).astype(np.uint8)


def neighbour_masks(n, db):
    """per pair (i, j) of the structure the mask over exactly its neighbours i - 1, j + 1, i + 1, j - 1 that exist and are unpaired
    in it (pairs without such a neighbour give no mask)"""
    out = []
    for i, j in pair_prob_ref.pairs_of(db):
        ps = [p for p in (i - 1, j + 1, i + 1, j - 1) if 1 <= p <= n and db[p - 1] == "."]
        if ps:
            out.append(ps)
    return mask_rows(n, out)


def inner_positions(n, seed, count=5):
    """positions 1, 2, n - 1, n and `count` seeded inner ones (1-based, ascending)"""
    rng = np.random.default_rng([SEED, 8, seed, n])
    return sorted({1, 2, n - 1, n} | {int(p) for p in rng.choice(np.arange(3, n - 1), size=count, replace=False)})


# ------------------------------------------------------------------------------------------------ cases

def sparse_cases():
    """name -> sequence: the twelve sparse cases of kbest_ref within the cap (100 - 260 nt; the two multiloop3_* are above it)"""
    return {k: v for k, v in kbest_ref.sparse_one_strand().items() if not k.startswith("multiloop3_")}


# Dense cases: seeded draws over pair_prob_ref.ALPHABETS, kept when the REFERENCE's largest opening energy over the masks the
# tests use exceeded 0.5 kcal/mol (a random 9-nt sequence often has no stem worth opening); the code under test played no part
DENSE_REFERENCE = ("GCGGAAGGC", "GCCGCGCCGG", "GGUCCCCCGAG", "GUGCCGGCAUAC", "CGGCGGCCCGCGG", "GCGGAAGAACUCUU", "CACUGCAAUGCCAGU",
                   "GCGGGCGCGGCGGCCC", "GCCCGCGCA", "UGGACGCCAUAC", "CCCCGCGCGCGGCG", "UAAGCGACUGGCGCGA")
DENSE_KERNEL = TIGHT + ("CGGGGGACC", "CGCGCCGGCCC", "AUGUCCAAGUGGU", "GUUCCUGCCAGCAGA")


def dense_reference_cases():
    """twelve sequences of 9 - 16 nt over pair_prob_ref.ALPHABETS"""
    return list(DENSE_REFERENCE)


def dense_kernel_cases():
    """six sequences of 9 - 16 nt: the two TIGHT ones and one each of 9, 11, 13 and 15 nt"""
    return list(DENSE_KERNEL)


def dense_masks(oracle, seq):
    """the mask set of a dense case: every single position, every window of 4, 20 seeded random masks and the neighbour masks of
    the MFE structure's pairs"""
    n = len(seq)
    parts = [single_masks(n), window_masks(n, 4), random_masks(n, 20, 0), neighbour_masks(n, oracle.mfe(seq)[0])]
    return np.concatenate([p for p in parts if p.shape[0]])


def check_case(ens, masks):
    """the conditions of a test case, on the reference alone: within the cap, counts equal (both raised by Ensemble) and a tested
    mask that costs more than MIN_EOPEN.  Returns F[mask]"""
    F = ens.free_energy(masks)
    if not (F - ens.F0).max() > MIN_EOPEN:
        raise ValueError("%s: no tested mask opens more than %.1f kcal/mol" % (ens.seq, MIN_EOPEN))
    return F
