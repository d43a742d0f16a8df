"""Constructed sequences that put ONE chosen loop into the minimum-free-energy structure (or, beyond the loop-size limit, just
out of it): every interior-loop shape up to 35 unpaired bases, the table-driven small loops over all closing pairs, hairpins
of 3 ... 70 bases and the tabulated special ones, multiloops of 2 ... 6 branches, and the two-strand and self-dimer forms.
Random sequences never fold into a 13 x 17 loop; these do, so a kernel that gets one shape wrong changes an answer.

A plain helper module (no fixtures, no pytest configuration).  Everything is generated from fixed rules and fixed seeds.
Records are (name, family, sequence, target, intended_loop); two-strand records carry '&' in sequence and target.
intended_loop holds 0-based positions in the sequence without the '&': (i, j, p, q) = outer pair (i, j) and inner pair (p, q)
of an interior loop or bulge, (i, j) = the closing pair of a hairpin, (i, j, k) = the closing pair and the branch count of a
multiloop."""
import gzip
import os
from collections import namedtuple

import numpy as np

Record = namedtuple("Record", "name family sequence target intended_loop")

MAXLOOP = 30
PAIRS = ("CG", "GC", "GU", "UG", "AU", "UA")
SMALL_SHAPES = ((0, 1), (1, 0), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 2), (1, 3), (3, 1), (1, 5))
NICKED_SIZES = (2, 8, 29, 30, 31, 32)
OFFSET_RULES = (0, 11, -1)              # the k of pad(): three placements of every record
_PAR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rna_turner1999.par.gz")


# ---- structure helpers

def pair_table(ss):
    """0-based partner of every position of a dot-bracket string ('&' removed), -1 = unpaired; '(' ')' only"""
    ss = ss.replace("&", "")
    pt, stk = [-1] * len(ss), []
    for i, ch in enumerate(ss):
        if ch == "(":
            stk.append(i)
        elif ch == ")":
            o = stk.pop()
            pt[o], pt[i] = i, o
    return pt


def has_loop(ss, rec, offset=0):
    """does the structure ss (of rec's sequence, placed `offset` bases to the right) contain rec's intended loop: its closing
    pairs present and nothing paired between them"""
    pt = pair_table(ss)
    lp = tuple(rec.intended_loop)
    if len(lp) == 4:
        i, j, p, q = (x + offset for x in lp)
        return pt[i] == j and pt[p] == q and all(pt[x] < 0 for x in range(i + 1, p)) and all(pt[x] < 0 for x in range(q + 1, j))
    if len(lp) == 2:
        i, j = (x + offset for x in lp)
        return pt[i] == j and all(pt[x] < 0 for x in range(i + 1, j))
    i, j, k = lp[0] + offset, lp[1] + offset, lp[2]
    if pt[i] != j:
        return False
    x, branches = i + 1, 0
    while x < j:
        if pt[x] > x:
            branches, x = branches + 1, pt[x] + 1
        elif pt[x] < 0:
            x += 1
        else:
            return False
    return branches == k


def shape_of(rec):
    """(u1, u2) of an interior-loop record; (loop length, 0) of the others"""
    lp = rec.intended_loop
    if len(lp) == 4:
        return lp[2] - lp[0] - 1, lp[1] - lp[3] - 1
    return lp[1] - lp[0] - 1, 0


def offset_of(rec, L, k):
    """left offset of rec inside a poly-A frame of total length L: a fixed rule of the shape, so that the loops of a family land
    on many residues mod 28, 32 and 64 (tower slots, ring rows, tower blocks), on offset 0 and flush right.  k >= 0:
    (7 u1 + 3 u2 + k) mod (room + 1) from the left end; k < 0: the same with -k - 1, counted from the right end"""
    n = len(rec.sequence)
    assert "&" not in rec.sequence and n <= L
    u1, u2 = shape_of(rec)
    room = L - n
    return (7 * u1 + 3 * u2 + k) % (room + 1) if k >= 0 else room - (7 * u1 + 3 * u2 - k - 1) % (room + 1)


def pad(rec, L, k=0, offset=None):
    """rec inside A...A of total length L -> (sequence, target, offset).  The constructs hold no U, or are closed by G-C
    helices, and poly-A pairs with nothing: the oracle checks that the answer stays the same."""
    off = offset_of(rec, L, k) if offset is None else offset
    n = len(rec.sequence)
    assert 0 <= off <= L - n
    return "A" * off + rec.sequence + "A" * (L - n - off), "." * off + rec.target + "." * (L - n - off), off


# ---- families

def interior_record(u1, u2):
    seq = "GGCG" + "A" * u1 + "GCGCGAAAGCGC" + "A" * u2 + "CGCC"
    tgt = "((((" + "." * u1 + "((((....))))" + "." * u2 + "))))"
    return Record("int_%dx%d" % (u1, u2), "interior", seq, tgt, (3, 16 + u1 + u2, 4 + u1, 15 + u1))


def interior(max_size=35):
    """every (u1, u2) with u1 + u2 <= max_size, stacked pair (0 x 0) and bulges included: 666 records for 35"""
    return [interior_record(u1, s - u1) for s in range(max_size + 1) for u1 in range(s + 1)]


def thinned_interior(max_size=35):
    """for the long frames: all shapes of sizes 0 - 7 and 28 - 32, and u1 = 0, 2, s // 2 of every other size"""
    out = []
    for s in range(max_size + 1):
        u1s = range(s + 1) if s <= 7 or 28 <= s <= 32 else sorted({0, 2, s // 2})
        out += [interior_record(u1, s - u1) for u1 in u1s]
    return out


def small_candidates(u1, u2, po, pi, seed=20260, limit=16):
    """the loop fillings tried for one shape and one (outer, inner) closing-pair combination: all 4^(u1+u2) of them when there
    are <= limit, else a seeded sample of limit"""
    m = u1 + u2
    total = 4 ** m
    if total <= limit:
        codes = list(range(total))
    else:
        rng = np.random.default_rng([seed, u1, u2, PAIRS.index(po), PAIRS.index(pi)])
        codes = sorted(int(x) for x in rng.choice(total, size=limit, replace=False))
    out = []
    for c in codes:
        fill = "".join("ACGU"[(c >> (2 * b)) & 3] for b in range(m))
        l1, l2 = fill[:u1], fill[u1:]
        seq = "GCC" + po[0] + l1 + pi[0] + "CGCGAAAGCG" + pi[1] + l2 + po[1] + "GGC"
        tgt = "(((" + "(" + "." * u1 + "(" + "(((....)))" + ")" + "." * u2 + ")" + ")))"
        i, p = 3, 4 + u1
        q = p + 11
        j = q + u2 + 1
        out.append(Record("small_%dx%d_%s_%s_%s" % (u1, u2, po, pi, fill or "-"), "small", seq, tgt, (i, j, p, q)))
    return out


def small(oracle=None, keep=16):
    """the table-driven shapes over all 36 closing-pair combinations, both closing pairs flanked by three G-C pairs.
    Without an oracle: every candidate filling (up to 16 per combination).  With one: per combination the first `keep`
    candidates whose MFE structure contains the intended loop (rejection sampling; the candidates and their order are fixed by
    the seeds), or the first candidate where none does, so that every combination stays represented."""
    out = []
    for u1, u2 in SMALL_SHAPES:
        for po in PAIRS:
            for pi in PAIRS:
                cand = small_candidates(u1, u2, po, pi)
                if oracle is not None:
                    hits = [r for r in cand if has_loop(oracle.mfe(r.sequence)[0], r)]
                    cand = hits[:keep] if hits else cand[:1]
                out += cand
    return out


def special_hairpins():
    """the tabulated tri-/tetra-/hexaloop entries (closing pair included) of the committed parameter file"""
    out, on = [], False
    with gzip.open(_PAR, "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                on = line.split()[1:2] in (["Triloops"], ["Tetraloops"], ["Hexaloops"])
                continue
            f = line.split()
            if on and len(f) == 3 and set(f[0]) <= set("ACGU"):
                out.append(f[0])
    return out


def hairpin():
    """loop lengths 3 ... 70 (beyond 30 the loop energy is extrapolated) and every special-loop entry"""
    out = []
    for h in range(3, 71):
        out.append(Record("hp_%d" % h, "hairpin", "GGCGC" + "A" * h + "GCGCC", "(((((" + "." * h + ")))))", (4, 5 + h)))
    for e in special_hairpins():
        n = len(e)
        out.append(Record("hp_special_" + e, "hairpin", "GGCG" + e + "CGCC", "((((" + "(" + "." * (n - 2) + ")" + "))))", (4, 3 + n)))
    return out


def multiloop(pinned=True):
    """k = 2 ... 6 branches; spacers a = 1, 2 are pinned (the oracle folds them into the k-branch multiloop), a = 0 is not"""
    out = []
    for a in ((1, 2) if pinned else (0,)):
        for k in range(2, 7):
            seq = "GGCGC" + ("A" * a + "GCGCGAAAGCGC") * k + "A" * a + "GCGCC"
            tgt = "(((((" + ("." * a + "((((....))))") * k + "." * a + ")))))"
            out.append(Record("ml_k%d_a%d" % (k, a), "multiloop" if pinned else "multiloop_unpinned", seq, tgt, (4, len(seq) - 5, k)))
    return out


def cofold_record(u1, u2, pad_b=0):
    a = "GGCG" + "A" * u1 + "GCGCG"
    b = "CGCGC" + "A" * u2 + "CGCC" + "A" * pad_b
    tgt = "((((" + "." * u1 + "(((((" + "&" + ")))))" + "." * u2 + "))))" + "." * pad_b
    return Record("co_%dx%d" % (u1, u2), "cofold", a + "&" + b, tgt, (3, 14 + u1 + u2, 4 + u1, 13 + u1))


def cofold(max_size=35, common=False):
    """the two-strand interior form, the nick in place of the hairpin.  common: second strands padded with A at their 3' end
    to 9 + max_size - u1, so that all pairs with the same u1 share their strand lengths (one call) and every pair is
    18 + max_size bases long"""
    return [cofold_record(u1, s - u1, (max_size - s) if common else 0) for s in range(max_size + 1) for u1 in range(s + 1)]


def nicked_record(u1, u2):
    h = u1 // 2
    a = "GGCG" + "A" * h
    b = "A" * (u1 - h) + "GCGCGAAAGCGC" + "A" * u2 + "CGCC"
    tgt = "((((" + "." * h + "&" + "." * (u1 - h) + "((((....))))" + "." * u2 + "))))"
    return Record("nick_%dx%d" % (u1, u2), "nicked", a + "&" + b, tgt, (3, 16 + u1 + u2, 4 + u1, 15 + u1))


def nicked():
    """the base construct with the nick inside the u1 run (after u1 // 2 bases): the would-be interior loop is an exterior
    loop, which has no size limit"""
    return [nicked_record(u1, s - u1) for s in NICKED_SIZES for u1 in sorted({1, s // 2, s}) if u1 >= 1]


def selfdimer(tail=0):
    """GGCC A^u GCGC A^u GGCC, u = 0 ... 17: both helices are self-complementary, so s & s forms symmetric u x u loops
    (sizes 0 ... 34); tail: A's appended"""
    out = []
    for u in range(18):
        s = "GGCC" + "A" * u + "GCGC" + "A" * u + "GGCC" + "A" * tail
        out.append(Record("sd_%d_t%d" % (u, tail), "selfdimer", s, "." * len(s), (0, len(s) - 1)))
    return out


def cut_of(rec):
    """length of the first strand (the oracle's cut), 0 for one strand"""
    return rec.sequence.index("&") if "&" in rec.sequence else 0
