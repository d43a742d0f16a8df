"""CPU check of the second-best co-fold kernel (desirna_amd/csrc/fold_cofold_subopt.hpp), compiled unmodified against the
HIP stand-in of tests/emu/ into a library of its own.  The reference pins no subopt output for two strands, so the kernel is
checked against explicit enumeration of every co-fold structure, each scored by the oracle's two-strand evaluation, and
against properties that follow from the structure set (unconnected-only pairs, homodimer rotation, bounds)."""
import numpy as np
import pytest

from tests.emu.emu import INF_REF, cofold_subopt, cofold_subopt_many

PAIRS = {("A", "U"), ("U", "A"), ("G", "C"), ("C", "G"), ("G", "U"), ("U", "G")}


def e2_rule(e12):
    """what the reference's -nd on takes: the second-best energy if it lies within 4900 dcal/mol of the MFE, else 0"""
    return e12[1] if e12[1] < INF_REF and e12[1] - e12[0] <= 4900 else 0


def cofold_structures(seq, cut):
    """every co-fold structure of the concatenation `seq` (first strand `cut` nt): canonical non-crossing pairs, a pair
    inside one strand encloses at least 3 nucleotides, a pair that joins the strands (i < cut <= j, 0-based) any number"""
    n = len(seq)
    out = []

    def rec(i, cur, stack):
        if i == n:
            if not stack:
                out.append("".join(cur))
            return
        cur.append(".")
        rec(i + 1, cur, stack)
        cur.pop()
        if n - i - 1 >= len(stack) + 1:
            cur.append("(")
            stack.append(i)
            rec(i + 1, cur, stack)
            stack.pop()
            cur.pop()
        if stack:
            o = stack[-1]
            if (i - o > 3 or o < cut <= i) and (seq[o], seq[i]) in PAIRS:
                stack.pop()
                cur.append(")")
                rec(i + 1, cur, stack)
                cur.pop()
                stack.append(o)

    rec(0, [], [])
    return out


def rotate(db, cut):
    """the structure of X&X seen with the strands swapped (positions rotated by cut)"""
    n = len(db)
    stack, pairs = [], []
    for k, ch in enumerate(db):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            pairs.append((stack.pop(), k))
    out = ["."] * n
    for i, j in pairs:
        a, b = sorted(((i + cut) % n, (j + cut) % n))
        out[a], out[b] = "(", ")"
    return "".join(out)


def _rand(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def _enumeration_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for k in range(60):
        la, lb = (int(x) for x in rng.integers(4, 9, size=2))
        alpha = ("ACGU", "GC", "AUUAGC")[k % 3]
        cases.append(_rand(rng, la, alpha) + "&" + _rand(rng, lb, alpha))
    return cases


@pytest.mark.parametrize("nt", [64, 128])
def test_two_best_against_enumeration(oracle, nt):
    cases = _enumeration_cases()
    got = cofold_subopt_many(cases, nt=nt)
    for s, (e2, e12, st) in zip(cases, got):
        assert st == 0, s
        la = len(s.split("&")[0])
        flat = s.replace("&", "")
        en = sorted(oracle.eval_structure(flat, db, la) for db in cofold_structures(flat, la))
        assert en[0] == oracle.cofold_mfe(s)[1], s                       # the structure set is the co-fold MFE's
        want = (en + [INF_REF])[:2]
        assert list(e12) == want, (s, nt)
        assert e2 == e2_rule(want), s


def test_unconnected_only_pairs(oracle):
    """nothing can join {G, C} to A: the structures are those of the G/C strand beside an unfoldable one, no DuplexInit
    (a kernel that also counted them as joined would report the ground state + DuplexInit as the second best)"""
    rng = np.random.default_rng(5)
    strands = [_rand(rng, la, "GC") for la in (9, 11, 13, 14)]
    cases = [x + "&" + "A" * lb for x, lb in zip(strands, (6, 4, 9, 12))]
    cases += ["A" * lb + "&" + x for x, lb in zip(strands, (5, 8, 4, 10))]       # mirrored
    got = cofold_subopt_many(cases + ["AAAA&AAAA"])
    for s, (e2, e12, st) in zip(cases, got):
        assert st == 0, s
        want = oracle.two_best(s.replace("&", "").strip("A") if s[0] == "A" else s.split("&")[0])
        assert e12 == want, s
        assert e2 == e2_rule(want), s
    e2, e12, st = got[-1]                                                 # one structure only (all unpaired)
    assert st == 0 and e12 == (0, INF_REF) and e2 == 0


def test_homodimer_rotation(oracle):
    """X&X: a ground state that is not its own rotation has a rotated twin of equal energy, counted as a second structure"""
    rng = np.random.default_rng(17)
    xs = []
    while len(xs) < 6:                          # strands whose co-fold ground state is not its own rotation (the oracle picks)
        x = _rand(rng, int(rng.integers(8, 13)), "GGCCAU")
        db = oracle.cofold_mfe(x + "&" + x)[0].replace("&", "")
        if rotate(db, len(x)) != db:
            xs.append(x)
    seqs = [x + "&" + x for x in xs]
    for s, x, (e2, e12, st) in zip(seqs, xs, cofold_subopt_many(seqs)):
        assert st == 0, s
        ss, e = oracle.cofold_mfe(s)
        rot = rotate(ss.replace("&", ""), len(x))
        assert oracle.eval_structure(s, rot, len(x)) == e, s            # the rotated twin: another structure, same energy
        assert e12 == (e, e) and e2 == e, s


def test_bounds_random(oracle):
    rng = np.random.default_rng(33)
    pairs = [(_rand(rng, la, alpha), _rand(rng, lb, alpha))
             for la, lb, alpha in ((12, 9, "ACGU"), (10, 10, "ACGU"), (13, 11, "GGCCAU"), (14, 12, "ACGU")) for _ in range(3)]
    got = cofold_subopt_many([a + "&" + b for a, b in pairs])
    for (a, b), (e2, e12, st) in zip(pairs, got):
        s = a + "&" + b
        assert st == 0, s
        assert e12[0] == oracle.cofold_mfe(s)[1], s
        (a1, a2), (b1, b2) = oracle.two_best(a), oracle.two_best(b)
        assert e12[0] <= e12[1] <= min(a1 + b2, a2 + b1), s
        assert e2 == e2_rule(e12)


def test_batch_and_bad_letter():
    """several pairs in one launch (workspace slots side by side) give the single-pair values; a bad letter is ST_BAD_CHAR"""
    seqs = ["GGGAAC&GUUCCC", "GCGCAU&AUGCGC", "GGGXAC&GUUCCC"]
    E2, E12, st = cofold_subopt(seqs, nt=64)
    assert list(st) == [0, 0, 1] and int(E2[2]) == 0
    for k, (e2, e12, s1) in enumerate(cofold_subopt_many(seqs[:2], nt=64)):
        assert (int(E2[k]), (int(E12[k, 0]), int(E12[k, 1]))) == (e2, e12)
