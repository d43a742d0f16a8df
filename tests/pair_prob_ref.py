"""Pair probabilities and ensemble defects WITHOUT an outside recursion: the reference of tests/test_pair_prob_reference.py and
tests/test_pair_prob_reference_gpu.py.  A plain helper module (no fixtures, no pytest configuration).

With F the ensemble free energy, F[not (i,j)] the free energy when the one pair (i,j) is forbidden and F[not i] the free energy
when i may pair with nothing (oracle.pf_forbid / oracle.cofold_pf_forbid: the inside fill with one condition on the pair-type
look-up), exactly

    P(i,j)      = 1 - exp(-(F[not (i,j)] - F) / kT)
    sum_j P(i,j) = 1 - exp(-(F[not i] - F) / kT)

because Z - Z[not (i,j)] is the weight of the structures that hold (i,j).  Two strands: F is FAB; expDuplexInit and the halving
for equal strands are weights of a STRUCTURE, so they are in Z and in Z[not ...] alike and the identity is untouched.  The
inside fills are pinned on the reference's golden Epf / FAB columns (tests/test_oracle_golden.py).  The defect of a target
takes one fill per base unpaired in the target and one per target pair: at most n.

Everything here looks at the oracle alone, never at the code under test."""
import numpy as np

PAIRS = {"AU", "UA", "GC", "CG", "GU", "UG"}
COMPLEMENT = {"A": "U", "U": "A", "G": "C", "C": "G"}
ALPHABETS = ("ACGU", "GC", "GGCCAU")


def rand_seq(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def split(seq):
    """'A&B' or 'A' -> (concatenation, cut); cut = 0 for one strand"""
    return seq.replace("&", ""), (seq.index("&") if "&" in seq else 0)


def pairs_of(db):
    db = db.replace("&", "")
    stk, out = [], []
    for k, ch in enumerate(db, 1):
        if ch == "(":
            stk.append(k)
        elif ch == ")":
            out.append((stk.pop(), k))
    return sorted(out)


def allowed_pairs(seq):
    """every (i, j), 1-based over the concatenation, that the loop model lets pair: canonical letters and, unless the pair joins
    the strands, at least three bases enclosed"""
    flat, cut = split(seq)
    n = len(flat)
    return [(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1)
            if flat[i - 1] + flat[j - 1] in PAIRS and (i <= cut < j or j - i >= 4)]


def reference_entries(oracle, seq, pairs):
    """float64[len(pairs)]: P_ref of each pair, one masked fill each"""
    return oracle.pair_probs_by_forbidding(seq, pairs=pairs)[0]


def reference_matrix(oracle, seq, pairs=None):
    """(n+1, n+1) upper-triangular, 1-based like the engine's; `pairs` None = every allowed pair, else only those are filled"""
    n = len(split(seq)[0])
    pairs = allowed_pairs(seq) if pairs is None else list(pairs)
    P = np.zeros((n + 1, n + 1))
    for (i, j), p in zip(pairs, reference_entries(oracle, seq, pairs)):
        P[i, j] = p
    return P


def reference_defect(oracle, seq, target):
    """(1/n) [ sum_{i unpaired in target} sum_j P(i,j) + sum_{(i,m) in target} 2 (1 - P(i,m)) ] from one masked fill per unpaired
    base and one per target pair.  A target pair the model cannot form has F[not (i,m)] = F, i.e. P = 0, as it must."""
    n = len(split(seq)[0])
    tp = pairs_of(target)
    paired = {k for p in tp for k in p}
    bases = [i for i in range(1, n + 1) if i not in paired]
    pp, rows = oracle.pair_probs_by_forbidding(seq, pairs=tp, bases=bases)
    return (rows.sum() + 2.0 * (1.0 - pp).sum()) / n


def two_strand_case(rng, la, lb, alphabet, planted):
    """'A&B' of random letters; planted: a reverse-complementary stretch of 6 to 10 nt (as long as the shorter strand allows)
    written across the strands at random offsets, so that pairs joining the strands carry weight"""
    a, b = list(rand_seq(rng, la, alphabet)), list(rand_seq(rng, lb, alphabet))
    k = int(rng.integers(6, 11))
    if planted:
        k = min(k, la, lb)
        oa, ob = int(rng.integers(0, la - k + 1)), int(rng.integers(0, lb - k + 1))
        b[ob:ob + k] = [COMPLEMENT[c] for c in reversed(a[oa:oa + k])]
    return "".join(a) + "&" + "".join(b)


def mfe_structure(oracle, seq):
    return oracle.cofold_mfe(seq)[0] if "&" in seq else oracle.mfe(seq)[0]


def sampled_pairs(oracle, seq, seed, per_line=None):
    """the sampled set of a long case, from the oracle and a seed alone: the pairs of the MFE structure, every allowed pair of 3
    random rows (i fixed, j > i) and of 3 random columns (j fixed, i < j) on the far side of the nick (one strand: of the second
    half).  per_line: where one masked fill is expensive (400 nt), a seeded draw of that many pairs from each row / column
    instead of all of them."""
    flat, cut = split(seq)
    n = len(flat)
    rng = np.random.default_rng(seed)
    allowed = allowed_pairs(seq)
    out = set(pairs_of(mfe_structure(oracle, seq)))
    rows = rng.choice(np.arange(1, (cut or n // 2) + 1), 3, replace=False)
    cols = rng.choice(np.arange((cut or n // 2) + 1, n + 1), 3, replace=False)
    for r in rows:
        line = [p for p in allowed if p[0] == r]
        out.update(line if per_line is None or len(line) <= per_line else [line[k] for k in rng.choice(len(line), per_line, replace=False)])
    for c in cols:
        line = [p for p in allowed if p[1] == c]
        out.update(line if per_line is None or len(line) <= per_line else [line[k] for k in rng.choice(len(line), per_line, replace=False)])
    return sorted(out)


def sample_is_informative(seq, pairs, p_ref):
    """the condition on a sampled set, on the reference values alone: at least 10 entries above 1e-3 (two strands: 3 of them
    joining the strands) and at least 5 below 1e-6"""
    cut = split(seq)[1]
    big = [p for p, v in zip(pairs, p_ref) if v > 1e-3]
    joining = [p for p in big if p[0] <= cut < p[1]]
    small = int((np.asarray(p_ref) < 1e-6).sum())
    return len(big) >= 10 and (cut == 0 or len(joining) >= 3) and small >= 5


def nested_target(n, cut=0, k=None, gap=4):
    """a target that is not all dots and owes nothing to the sequence: k pairs (x, n + 1 - x) from the ends inwards"""
    k = max(0, min(k if k is not None else n // 4, (n - gap) // 2 if not cut else min(cut, n - cut)))
    return "(" * k + "." * (n - 2 * k) + ")" * k
