"""Reference of the two-strand stochastic traceback's tests (tests/test_cofold_sampling_emulated.py,
tests/test_cofold_sampling_gpu.py): the exact distribution over every co-fold structure of a short pair, by enumeration, in the
ensemble of DESIGN 3.5 -- a structure weighs exp(-E / kT) with the oracle's two-strand evaluation (DuplexInit included for a
connected structure), halved for a connected structure of two equal strands.  This is the enumeration of
tests/test_cofold_edef_emulated.py::enumerate_ensemble.  A plain helper module (no fixtures, no pytest configuration); it looks
at the oracle alone, never at the code under test."""
import math

from tests.pair_prob_ref import PAIRS, pairs_of, split
from tests.sampling_ref import KT
from tests.test_cofold_subopt_emulated import cofold_structures, rotate

# (pair, structures in the enumeration): every one enters the exact tests -- |F_enum - oracle.cofold_pf(s)[3]| < 1e-6 kcal/mol,
# i.e. the integer evaluation and the partition function's smoothed loop model agree (checked by the tests, case by case)
NAMED = [
    ("UAGAUUAC&AGAA", 62),
    ("ACAGAAUU&GUCA", 53),
    ("UGUAA&CUAUAUCA", 172),
    ("GCUUAAAC&UUAGAACC", 657),
    ("CUCGG&AAAGUCUG", 102),
    ("GCAGCGAAAGCAGG&CCAGCGAAAGC", 6150),
    ("GGUGUUA&GGUGUUA", 474),
    ("GCUCAU&GCUCAU", 49),
    ("GCUGUUA&GCUGUUA", 280),
    ("AAACGG&AAACGG", 9),
]
MULTILOOP = "GCAGCGAAAGCAGG&CCAGCGAAAGC"
ENTRY_TOL = 1e-6


def with_nick(db, cut):
    return db[:cut] + "&" + db[cut:]


def is_connected(db, cut=None):
    """some pair joins the strands; db with '&', or without it and cut given"""
    if cut is None:
        cut = db.index("&")
    return any(i <= cut < j for i, j in pairs_of(db))


def exact_weights(oracle, pair):
    """{structure with '&': weight} over the whole enumeration"""
    flat, cut = split(pair)
    homo = flat[:cut] == flat[cut:]
    out = {}
    for db in cofold_structures(flat, cut):
        w = math.exp(-oracle.eval_structure(flat, db, cut) / 100.0 / KT)
        if homo and is_connected(db, cut):
            w *= 0.5
        out[with_nick(db, cut)] = w
    return out


def exact_distribution(oracle, pair):
    """({structure with '&': p}, F_enum in kcal/mol); the probabilities sum to 1"""
    w = exact_weights(oracle, pair)
    Z = sum(w.values())
    return {s: v / Z for s, v in w.items()}, -KT * math.log(Z)


def enters(oracle, pair, F_enum):
    return abs(F_enum - oracle.cofold_pf(pair)[3]) < ENTRY_TOL


def connected_fraction(oracle, pair):
    """exp(-(FcAB - FAB) / kT) from the oracle's fill"""
    F4 = oracle.cofold_pf(pair)
    return math.exp(-(F4[2] - F4[3]) / KT)


def rotated(db):
    """the structure of X&X (with '&') seen with the strands swapped"""
    cut = db.index("&")
    return with_nick(rotate(db.replace("&", ""), cut), cut)


def well_formed(pair, db):
    """db carries the '&' where the pair does; balanced; canonical pairs; a pair inside a strand encloses at least three bases"""
    if len(db) != len(pair) or db.count("&") != 1 or db.index("&") != pair.index("&") or set(db) - set("().&"):
        return False
    flat, cut = split(pair)
    stk = []
    for k, ch in enumerate(db.replace("&", ""), 1):
        if ch == "(":
            stk.append(k)
        elif ch == ")":
            if not stk:
                return False
            o = stk.pop()
            if flat[o - 1] + flat[k - 1] not in PAIRS or not (o <= cut < k or k - o > 3):
                return False
    return not stk


def nick_multiloop_share(dist):
    """mass of the structures in which a JOINING pair closes a multiloop (>= 2 inner stems, the nick inside one of them)"""
    tot = 0.0
    for db, p in dist.items():
        cut = db.index("&")
        prs = pairs_of(db)
        for i, j in prs:
            if not i <= cut < j:
                continue
            inner = [(a, b) for a, b in prs if i < a and b < j and not any(i < c < a and b < e < j for c, e in prs)]
            if len(inner) >= 2 and any(a <= cut < b for a, b in inner):
                tot += p
                break
    return tot
