"""Reference of the MEA / centroid tests (tests/test_mea_reference.py, test_mea_emulated.py, test_mea_gpu.py) in plain numpy: the
recurrence as the contract states it, WITHOUT the kernel's pruning, with the tie rule; the expected accuracy of a given structure;
the centroid and its distance; an exhaustive maximiser over an enumeration of structures.  A plain helper module (no fixtures, no
pytest configuration); it never looks at the code under test.

P is an (n+1, n+1) array, P[i, j] for 1 <= i < j <= n (what drna_ensemble_defect_batch returns in bpp); everything else is ignored.

    q(i)    = 1 - sum_j P(min(i,j), max(i,j))        summed in ascending j, not clamped
    EA(s)   = sum_{i unpaired in s} q(i) + 2 gamma sum_{(i,j) in s} P(i,j)
    M(i,i-1) = 0,  M(i,j) = max( M(i,j-1) + q(j), max_{i <= k < j, P(k,j) > 0} M(i,k-1) + M(k+1,j-1) + 2 gamma P(k,j) )
    tie rule: "j unpaired" first, then k ascending; a later candidate replaces only if strictly greater

Tolerance (derived, not measured): a value is a sum of at most n terms, each a sum of at most n doubles of size at most
max(1, 2 gamma), so two correct evaluations differ by at most tol(n, gamma) = 2 n^2 2^-53 (1 + 2 gamma)."""
import numpy as np

from tests.pair_prob_ref import pairs_of


def tol(n, gamma):
    return 2.0 * n * n * 2.0 ** -53 * (1.0 + 2.0 * gamma)


def unpaired_probs(P):
    """q[1..n] (q[0] unused)"""
    n = P.shape[0] - 1
    q = np.zeros(n + 1)
    for i in range(1, n + 1):
        s = 0.0
        for j in range(1, n + 1):
            if j != i:
                s += float(P[min(i, j), max(i, j)])
        q[i] = 1.0 - s
    return q


def mea(P, gamma):
    """(structure as dot-bracket, value M(1,n)) by the recurrence, every candidate with P > 0 visited.  The candidates of a cell are
    evaluated elementwise, (M(i,k-1) + M(k+1,j-1)) + 2 gamma P(k,j) each, and np.argmax takes the FIRST greatest: k ascending, a
    later one only if strictly greater."""
    n = P.shape[0] - 1
    q = unpaired_probs(P)
    M = np.zeros((n + 2, n + 2))                      # M[i, j], M[i, i-1] = 0
    ks = [np.array([k for k in range(1, j) if P[k, j] > 0.0], dtype=np.int64) for j in range(n + 1)]
    ws = [2 * gamma * P[ks[j], j] for j in range(n + 1)]

    def best(i, j):
        v, kb = M[i, j - 1] + q[j], 0
        a = int(np.searchsorted(ks[j], i))
        if a < len(ks[j]):
            k = ks[j][a:]
            c = M[i, k - 1] + M[k + 1, j - 1] + ws[j][a:]
            x = int(np.argmax(c))
            if c[x] > v:
                v, kb = c[x], int(k[x])
        return v, kb

    for length in range(1, n + 1):
        for i in range(1, n - length + 2):
            j = i + length - 1
            M[i, j] = best(i, j)[0]
    db = ["."] * n
    todo = [(1, n)]
    while todo:
        i, j = todo.pop()
        while j >= i:
            _, k = best(i, j)
            if k == 0:
                j -= 1
                continue
            db[k - 1], db[j - 1] = "(", ")"
            todo.append((k + 1, j - 1))
            j = k - 1
    return "".join(db), float(M[1, n])


def expected_accuracy(P, db, gamma):
    """EA_gamma of the structure db ('&' ignored)"""
    db = db.replace("&", "")
    q = unpaired_probs(P)
    prs = pairs_of(db)
    paired = {x for p in prs for x in p}
    ea = 0.0
    for i in range(1, len(db) + 1):
        if i not in paired:
            ea += q[i]
    for i, j in prs:
        ea += 2 * gamma * float(P[i, j])
    return ea


def centroid(P):
    """(dot-bracket of {P > 0.5}, its distance sum_{c} (1 - P) + sum_{not c} P)"""
    n = P.shape[0] - 1
    db = ["."] * n
    d = 0.0
    for i in range(1, n + 1):
        for j in range(i + 1, n + 1):
            p = float(P[i, j])
            if p > 0.5:
                assert db[i - 1] == "." and db[j - 1] == ".", "two pairs of probability above one half share a base"
                db[i - 1], db[j - 1] = "(", ")"
                d += 1.0 - p
            else:
                d += p
    return "".join(db), d


def exhaustive_max(P, structures, gamma):
    """the largest EA_gamma over the given dot-bracket strings whose pairs all have P > 0"""
    best = None
    for db in structures:
        if all(P[i, j] > 0.0 for i, j in pairs_of(db)):
            v = expected_accuracy(P, db, gamma)
            if best is None or v > best:
                best = v
    return best


def synthetic_matrix(n, seed, density=0.5, unit=8):
    """a matrix (its pairs may cross) whose entries are multiples of 1/unit (unit a power of two) with row sums <= 1: every sum
    the recurrence forms is exact in fp64 (for gamma a power of two), so string and value are fixed to the bit by the contract
    alone.  No hairpin rule: any i < j."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n + 1, n + 1))
    left = np.full(n + 1, unit, dtype=np.int64)       # units each base can still give away
    tries = int(density * n * 4) + 1
    for _ in range(tries):
        if n < 2:
            break
        i, j = sorted(int(x) for x in rng.integers(1, n + 1, size=2))
        if i == j or P[i, j] > 0:
            continue
        m = int(min(left[i], left[j]))
        if m < 1:
            continue
        e = int(rng.integers(1, m + 1))
        P[i, j] = e / float(unit)
        left[i] -= e
        left[j] -= e
    return P


def band_matrix(n, band, unit):
    """every pair 1 <= j - i <= band with probability 1 / unit (2 band <= unit, a power of two): rows sum to 2 band / unit away from
    the ends, so with 2 gamma / unit >= 2 no pair is pruned and a column holds `band` candidates; exact sums as synthetic_matrix"""
    assert 2 * band <= unit
    P = np.zeros((n + 1, n + 1))
    for i in range(1, n + 1):
        for j in range(i + 1, min(n, i + band) + 1):
            P[i, j] = 1.0 / unit
    return P


def eterna_by_length(eterna_solutions, lengths):
    """the first golden Eterna solution of each length: [(sequence, structure), ...]"""
    by_len = {}
    for r in eterna_solutions:
        by_len.setdefault(len(r["sequence"]), (r["sequence"], r["structure"]))
    return [by_len[n] for n in lengths]


def well_formed(P, db):
    """balanced ( ) . of the matrix's length (an '&' anywhere is ignored), every pair with P > 0"""
    db = db.replace("&", "")
    if len(db) != P.shape[0] - 1 or set(db) - set("()."):
        return False
    depth = 0
    for ch in db:
        depth += ch == "("
        depth -= ch == ")"
        if depth < 0:
            return False
    return depth == 0 and all(P[i, j] > 0.0 for i, j in pairs_of(db))
