"""Cases and the comparison rule for the ranked-structure (K-best) folds, one and two strands.

A plain helper module (no fixtures, no pytest configuration), used by tests/test_kbest_reference.py (CPU) and
tests/test_kbest_reference_gpu.py.  Two references, both in oracle/oracle.c:

    oracle.enum_kbest(seq, K)       every structure of the sequence (or pair, 'A&B'), each scored by eval_structure: the root
                                    of trust, affordable while count_structures(seq) <= CAP
    oracle.kbest_energies(seq, K)   the serial K-list fill (energies only), any length; held to enum_kbest on every case here

Dense cases are short random sequences.  SPARSE cases are long: a background of A (no U anywhere, so A pairs with nothing) with a
few G / C letters, which alone can pair; enumeration is then exact at 100 - 260 nt, with hairpins longer than 30, interior loops at
MAXLOOP, multiloops with long unpaired runs and split spans beyond one wave of 64 lanes.  All cases come from fixed seeds.
"""
import numpy as np

INF_REF = 10000000
CAP = 5_000_000                     # structures per enumerated case
MAXLOOP = 30
SEED = 20260


def _rand(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def _fill(L, *parts):
    """parts laid out left to right, padded with A at the 3' end to L"""
    s = "".join("A" * p if isinstance(p, int) else p for p in parts)
    assert len(s) <= L, (len(s), L)
    return s + "A" * (L - len(s))


# ------------------------------------------------------------------------------------------------ dense cases

ONE_STRUCTURE_MORE = "AAGAAAACAA"           # the open chain and G3-C8, nothing else


# named cases: short sequences on which a planted mistake in the kernels' list handling changes a rank that random sequences
# of this size leave alone (found with the same mistakes planted in the oracle fill).  The first two are a multiloop with unpaired
# bases before its closing helix: the M2[i,j-1] + b term carries ranks >= 2 there; all four need list ranks a + b = K - 1 of a
# two-list sum (lists of 4: the first two; lists of 8: the last two)
NAMED_ONE = {
    "multiloop_tail_29": "GGGAGGGAAACCCAGGGAAACCCAAACCC",
    "multiloop_tail_30": "GGAGGGAAAACCCAGGGAAAACCCAAAACC",
    "full_lists_28": "CCGGUAACGGCUGCCCCAGUUAGCCGGA",
    "full_lists_25": "CAAAGGCGGCACCAUAGCCCGGCCG",
}


# the same for two strands: pairs on which a skipped update of the exterior lists next to the nick (fcB on diagonals 5, 6 or 8,
# fcA on diagonal 8) changes a rank: a helix that joins the strands encloses a short hairpin right after (before) the nick.
# The first is a sparse 20+44 with the nick far from both ends
NAMED_TWO = {
    "nick_lists_20+44": _fill(20, 6, "GGGG", 10) + "&" + _fill(44, "GAAAAC", 8, "CCCC", 10, "GGGAAAACCC"),
    "nick_lists_12+16": "AAGGGAGAAAAC&GAAAACAACCCAAAAA",
    "nick_lists_11+12": "AGUCCGAUAUG&CGUGAGAGAUGG",
    "nick_lists_11+10": "GCGACAAACCG&GCCAACAGCG",
}


def dense_one_strand():
    """35 sequences of 18 - 30 nt over ACGU, GC and GGCCAU, the named cases, A*12 and a sequence with one structure besides the open chain"""
    rng = np.random.default_rng([SEED, 1])
    out = []
    for k in range(33):
        alpha = ("ACGU", "GC", "GGCCAU")[k % 3]
        L = int(rng.integers(18, 31)) if alpha == "ACGU" else int(rng.integers(18, 27))
        out.append(_rand(rng, L, alpha))
    out += [_rand(rng, 30), _rand(rng, 30)]
    return out + list(NAMED_ONE.values()) + ["A" * 12, ONE_STRUCTURE_MORE]


def dense_two_strands():
    """30 pairs from 6+6 to 14+14, the unequal 3+20, 20+3, 1+24, 24+1, two X&X homodimers and the named cases"""
    rng = np.random.default_rng([SEED, 2])
    out = []
    for k in range(30):
        alpha = ("ACGU", "GGCCAU", "ACGU")[k % 3]
        la, lb = (int(x) for x in rng.integers(6, 15 if alpha == "ACGU" else 12, size=2))
        out.append(_rand(rng, la, alpha) + "&" + _rand(rng, lb, alpha))
    out.append(_rand(rng, 14) + "&" + _rand(rng, 14))
    for la, lb in ((3, 20), (20, 3), (1, 24), (24, 1)):
        out.append(_rand(rng, la) + "&" + _rand(rng, lb))
    for L in (9, 12):
        x = _rand(rng, L, "GGCCAU")
        out.append(x + "&" + x)
    return out + list(NAMED_TWO.values())


# ------------------------------------------------------------------------------------------------ sparse long cases

def _sparse(rng, L, letters):
    """A * L with `letters` G / C letters in runs of 2 - 4 at seeded places (runs never touch)"""
    s = ["A"] * L
    left, k = letters, 0
    while left > 0:
        run = min(left, int(rng.integers(2, 5)))
        if left - run == 1:
            run += 1
        p = int(rng.integers(1, L - run - 1))
        if any(ch != "A" for ch in s[p - 1:p + run + 1]):
            continue
        s[p:p + run] = "GC"[k % 2] * run                  # G and C runs in turn: about as many of each
        left -= run
        k += 1
    return "".join(s)


# hand-placed.  H = "GGG" + A*4 + "CCC" is a hairpin; stems of G on the 5' side and C on the 3' side only
_H, _H2 = "GGGAAAACCC", "GGAAAACC"
SPARSE_HAND_ONE = {
    # closing stem, three hairpins 26 / 45 nt apart (a three-stem multiloop that spans 93 / 161 nt: the split loops run a second
    # and a third pass).  20 and 22 letters: more than the seeded cases hold, still within CAP
    "multiloop3_130": _fill(130, 2, "GG", 6, _H, 26, _H, 26, _H2, 6, "CC"),
    "multiloop3_260": _fill(260, 40, "GG", 20, _H, 45, _H, 45, _H, 20, "CC"),
    # two helices joined by an interior loop of exactly MAXLOOP, one under, one over (the last cannot form)
    "interior30_100": _fill(100, 5, "GGGG", 15, "GGG", 4, "CCC", 15, "CCCC"),
    "interior29_100": _fill(100, 5, "GGGG", 15, "GGG", 4, "CCC", 14, "CCCC"),
    "interior31_100": _fill(100, 5, "GGGG", 16, "GGG", 4, "CCC", 15, "CCCC"),
    "bulge30_100": _fill(100, 5, "GGGG", 30, "GGG", 4, "CCC", "CCCC"),
    # hairpin loops of 35 and 70
    "hairpin35_200": _fill(200, 20, "GGGG", 35, "CCCC", 30, "GGG", 70, "CCC"),
}


def sparse_one_strand():
    """name -> sequence: seeded placements at 100, 130, 200 and 260 nt (12 - 16 letters) and the hand-placed ones"""
    out = {}
    for L, letters, seed in ((100, 12, 0), (100, 14, 1), (130, 13, 2), (200, 14, 3), (200, 16, 4), (260, 12, 5), (260, 15, 6)):
        out["seeded_%d_%d" % (L, letters)] = _sparse(np.random.default_rng([SEED, 3, seed]), L, letters)
    out.update(SPARSE_HAND_ONE)
    return out


SPARSE_HAND_TWO = {
    # the closing pair joins the strands; the multiloop's three stems: a hairpin in each strand and a helix that encloses the nick
    "multiloop3_nick_50+50": _fill(50, 2, "GG", 5, _H, 5, "GG", 6) + "&" + _fill(50, 6, "CC", 5, _H, 5, "CC"),
    "multiloop3_nick_30+170": _fill(30, 2, "GG", 3, _H, 3, "GGG", 2) + "&" + _fill(170, 4, "CCC", 30, _H, 60, "CC"),
    # interior loop of MAXLOOP between two helices that join the strands
    "interior30_50+50": _fill(50, 10, "GGGG", 15, "GGG", 3) + "&" + _fill(50, 3, "CCC", 15, "CCCC"),
}


def sparse_two_strands():
    out = {}
    for la, lb, letters, seed in ((50, 50, 12, 0), (50, 50, 14, 1), (100, 100, 13, 2), (100, 100, 15, 3), (30, 170, 14, 4), (170, 30, 12, 5)):
        s = _sparse(np.random.default_rng([SEED, 4, seed]), la + lb, letters)
        out["seeded_%d+%d_%d" % (la, lb, letters)] = s[:la] + "&" + s[la:]
    out.update(SPARSE_HAND_TWO)
    return out


# ------------------------------------------------------------------------------------------------ GPU case lists

GPU_LENGTHS = (24, 36, 63, 64, 65, 100, 129, 200, 260)
GPU_PAIR_SHAPES = ((14, 14), (18, 18), (17, 40), (40, 17), (50, 50), (100, 100), (1, 35), (35, 1))


def gpu_one_strand(L):
    """five sequences of L nt: random ACGU, GC, GGCCAU, A*L and a sparse one"""
    rng = np.random.default_rng([SEED, 5, L])
    return [_rand(rng, L), _rand(rng, L, "GC"), _rand(rng, L, "GGCCAU"), "A" * L, _sparse(rng, L, 12)]


def gpu_two_strands(la, lb):
    rng = np.random.default_rng([SEED, 6, la, lb])
    return [_rand(rng, la) + "&" + _rand(rng, lb), _rand(rng, la, "GC") + "&" + _rand(rng, lb, "GC"),
            _rand(rng, la, "GGCCAU") + "&" + _rand(rng, lb, "GGCCAU"), "A" * la + "&" + "A" * lb]


def gpu_homodimer(L=30):
    x = _rand(np.random.default_rng([SEED, 7, L]), L, "GGCCAU")
    return x + "&" + x


# ------------------------------------------------------------------------------------------------ the comparison rule

def balanced(db):
    depth = 0
    for ch in db:
        if ch not in "().":
            return False
        depth += (ch == "(") - (ch == ")")
        if depth < 0:
            return False
    return depth == 0


def check_ranked(oracle, seq, E, ss, ref_E, ref_ss=None):
    """The one rule every ranked answer is held to.  seq: the sequence ('A&B' for two strands); E, ss: the K returned energies and
    strings ('&' in the strings is ignored); ref_E: at least K reference energies (oracle.kbest_energies or oracle.enum_kbest);
    ref_ss: the strings of oracle.enum_kbest where enumeration ran.
      (a) the returned energies equal the reference's first K exactly, padding included;
      (b) the finite strings are balanced, pairwise distinct and worth the energy reported for them (oracle.eval_structure);
          padded ranks are all dots;
      (c) with ref_ss: every enumerated structure strictly below the last finite returned energy is among the returned strings
          (structures tied at the last energy may be any of the tied ones: their order is the engine's own)."""
    K = len(E)
    E = [int(e) for e in E]
    flat = seq.replace("&", "")
    cut = seq.index("&") if "&" in seq else 0
    strs = [x.replace("&", "") for x in ss]
    assert len(strs) == K and len(ref_E) >= K, (seq, K)
    assert E == [int(e) for e in ref_E[:K]], (seq, E, list(ref_E[:K]))                                   # (a)
    fin = [x for e, x in zip(E, strs) if e < INF_REF]
    assert len(set(fin)) == len(fin), (seq, fin)                                                           # (b)
    for e, x in zip(E, strs):
        assert len(x) == len(flat), (seq, x)
        if e >= INF_REF:
            assert x == "." * len(flat), (seq, x)
        else:
            assert balanced(x), (seq, x)
            assert oracle.eval_structure(flat, x, cut) == e, (seq, x, e)
    if ref_ss is not None and fin:                                                                        # (c)
        last = max(e for e in E if e < INF_REF)
        for e, x in zip(ref_E, ref_ss):
            if e < last:
                assert x in fin, (seq, x, e)


# ------------------------------------------------------------------------------------------------ structure features

def pair_table(db):
    pt, stk = {}, []
    for k, ch in enumerate(db):
        if ch == "(":
            stk.append(k)
        elif ch == ")":
            o = stk.pop()
            pt[o], pt[k] = k, o
    return pt


def loops(db, cut=0):
    """[(kind, size, stems, span)] of every loop closed by a pair: kind 'H', 'I' (interior, bulge or stack), 'M' or 'N' (the loop
    that holds the nick); size = unpaired nucleotides in it, stems = helices inside, span = j - i"""
    pt = pair_table(db)
    out = []
    for i in sorted(pt):
        j = pt[i]
        if j < i:
            continue
        stems, unp, p, nick = 0, 0, i + 1, cut > 0 and i < cut <= j
        while p < j:
            if pt.get(p, -1) > p:
                if p < cut <= pt[p]:
                    nick = False
                stems += 1
                p = pt[p] + 1
            else:
                unp += 1
                p += 1
        out.append(("N" if nick else "H" if stems == 0 else "I" if stems == 1 else "M", unp, stems, j - i))
    return out
