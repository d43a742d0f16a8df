"""The CPU oracle under the probe parameter sets of tests/probe_params.py, against the definition: every secondary structure of
a short sequence is enumerated and scored by the oracle's structure walks (eval_structure, boltzmann_weight), and the dynamic
programmes (mfe, pf, ensemble_defect, two_best, cofold_mfe, cofold_pf) must agree with the enumeration.  The GPU and emulated
parity tests under the probes compare against this oracle, so this module is what pins it where Turner-1999 cannot."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import probe_params as PP
from tests.test_cofold_subopt_emulated import cofold_structures
from tests.test_oracle_golden import ENUM_FIXED, KT, _enumerate, _pairs_of

INF_REF = 10000000


def test_turner1999_has_every_degeneracy():
    """the record of why the probe exists"""
    P = PP.turner_dict()
    PP.assert_has_degeneracies(P)
    assert (len(P["Triloops"]), len(P["Tetraloops"]), len(P["Hexaloops"])) == (0, 30, 0)
    assert np.array_equal(PP.probe_blob("turner1999"), PP.params.build_blob(P))     # the shipped blob is this file


def test_distinct_probe_breaks_every_degeneracy():
    P = PP.probe_dict("distinct")
    PP.assert_breaks_degeneracies(P)
    T = PP.turner_dict()
    for k in PP.LOOP_TABLES + PP.DANGLE_TABLES:
        inf = np.abs(T[k]) >= PP.params.INF // 2
        assert np.array_equal(P[k][inf], T[k][inf]) and np.abs(P[k][~inf] - T[k][~inf]).max() <= 60, k     # INF stays INF
    assert P["ninio"] < P["max_ninio"]
    assert np.array_equal(PP.probe_blob("distinct"), PP.params.build_blob(PP.probe_dict("distinct")))      # deterministic


def test_full_special_probe_fills_the_lists():
    tri, tetra, hexa = PP.special_loops("full_special")
    for lst, n in ((tri, 5), (tetra, 6), (hexa, 8)):
        assert len(lst) == PP.MAX_SPECIAL == len({s for s, _ in lst}) and all(len(s) == n for s, _ in lst)
        assert all(s[0] + s[-1] in PP.PAIRS for s, _ in lst)
    assert tetra[:30] == PP.turner_dict()["Tetraloops"]
    assert len({e for _, e in tri}) == 64 and len({e for _, e in hexa}) == 64 and len({e for _, e in tetra[30:]}) == 34


def _cases(name):
    rng = np.random.default_rng(55)
    cases = list(ENUM_FIXED) + [PP.TRI_HAIRPIN, PP.HEXA_HAIRPIN, PP.MULTILOOP]
    for trial in range(20):
        L = int(rng.integers(10, 18))
        cases.append(("".join(rng.choice(list("ACGU" if trial % 3 else "GC"), L)), None))
    if name == "full_special":
        for lst in PP.special_loops(name):
            cases += [PP.special_hairpin(lst[0][0]), PP.special_hairpin(lst[-1][0])]
    return cases


@pytest.fixture(scope="module", params=["distinct", "full_special"])
def probe(request):
    pyoracle.build()
    return request.param, pyoracle.Oracle(PP.probe_blob(request.param))


def test_oracle_against_enumeration(probe):
    """MFE = min E(structure) and E(mfe_ss) = Emfe; pf against the summed boltzmann_weight to 1e-11; pair probabilities and the
    defect to 1e-12; the two lowest energies exactly.  The census makes sure that the ensembles hold the loops the probe is
    about: special tri- and hexaloops, multiloops with unpaired bases, 1 x n and 2 x 3 interior loops."""
    name, orc = probe
    tri, tetra, hexa = ({s for s, _ in lst} for lst in PP.special_loops(name))
    seen = dict(tri=0, hexa=0, multi_unpaired=0, one_n=0, two_three=0)
    for seq, target in _cases(name):
        n = len(seq)
        structs = _enumerate(seq, orc)
        en = [orc.eval_structure(seq, st) for st in structs]
        ss, e = orc.mfe(seq)
        assert e == min(en) and orc.eval_structure(seq, ss) == e, seq
        srt = sorted(en)
        assert orc.two_best(seq) == (srt[0], srt[1] if len(srt) > 1 else INF_REF), seq
        w = np.array([orc.boltzmann_weight(seq, st) for st in structs])
        assert (w > 0).all()
        Z = w.sum()
        assert abs(-KT * np.log(Z) - orc.pf(seq)) < 1e-11, seq
        P = np.zeros((n, n))
        for st, wi in zip(structs, w):
            prs = _pairs_of(st)
            for (i, j) in prs:
                P[i, j] += wi
                inner = [(p, q) for (p, q) in prs if i < p and q < j and not any(i < a < p and q < b < j for (a, b) in prs)]
                if not inner:
                    seen["tri"] += j - i == 4 and seq[i:j + 1] in tri
                    seen["hexa"] += j - i == 7 and seq[i:j + 1] in hexa
                elif len(inner) >= 2:
                    seen["multi_unpaired"] += (j - i - 1) > sum(q - p + 1 for p, q in inner)
                else:
                    u = sorted((inner[0][0] - i - 1, j - inner[0][1] - 1))
                    seen["one_n"] += u[0] == 1 and u[1] >= 3
                    seen["two_three"] += u == [2, 3]
        P /= Z
        tgt = target or structs[int(np.argmax(w))]
        ed, bpp = orc.ensemble_defect(seq, tgt, want_bpp=True)
        assert np.abs(bpp[1:, 1:] - P).max() < 1e-12, seq
        pi = P.sum(axis=0) + P.sum(axis=1)
        paired = {}
        for (i, j) in _pairs_of(tgt):
            paired[i], paired[j] = (i, j), (i, j)
        want = sum((1.0 - P[paired[k]]) if k in paired else pi[k] for k in range(n)) / n
        assert abs(ed - want) < 1e-12, (seq, tgt)
        assert abs(orc.ensemble_defect(seq, "." * n) - pi.sum() / n) < 1e-12, seq
    assert all(seen.values()), seen


def test_special_hairpins_take_their_tabulated_energy(probe):
    """a hairpin closed by a tabulated loop string: E(structure) differs from the same helix around an untabulated loop of the
    same size by exactly what the table says (tri: the entry replaces size term + terminal-AU; tetra / hexa: it replaces the
    whole loop) -- here only that first and last entry of every list are FOUND: the evaluation changes when the entry's energy
    does"""
    name, orc = probe
    for which, lst in zip(("Triloops", "Tetraloops", "Hexaloops"), PP.special_loops(name)):
        if not lst:
            continue
        for k in (0, len(lst) - 1):
            P = PP.probe_dict(name)
            s, e = P[which][k]
            P[which][k] = (s, e + 37)
            moved = pyoracle.Oracle(PP.params.build_blob(P))
            seq, tgt = PP.special_hairpin(s)
            assert moved.eval_structure(seq, tgt) - orc.eval_structure(seq, tgt) == 37, (which, k)
            assert abs(np.log(orc.boltzmann_weight(seq, tgt) / moved.boltzmann_weight(seq, tgt)) * KT - 0.37) < 1e-12, (which, k)


def _clamp_smooth_gap():
    """the largest difference, in dcal/mol, between the MFE's min(0, x) and the partition function's -smooth(-x) over the integer
    dangle-like energies x (ViennaRNA's SMOOTH): the two loop models differ by at most this per dangle-like term"""
    def smooth(x):
        if x / 10.0 < -1.2283697:
            return 0.0
        if x / 10.0 > 0.8660254:
            return x
        s = np.sin(x / 10.0 - 0.34242663) + 1.0
        return 10.0 * 0.38490018 * s * s
    return max(abs(min(0, x) + smooth(-x)) for x in range(-400, 401))


def _cofold_cases():
    rng = np.random.default_rng(2025)
    cases = []
    for k in range(24):
        la, lb = (int(x) for x in rng.integers(4, 9, size=2))
        alpha = ("ACGU", "GC", "AUUAGC")[k % 3]
        a = "".join(rng.choice(list(alpha), la))
        cases.append(a + "&" + (a if k % 8 == 7 else "".join(rng.choice(list(alpha), lb))))
    return cases


@pytest.mark.parametrize("name", ["distinct_sharp", "distinct", "full_special"])
def test_cofold_against_enumeration(name):
    """two strands: cofold_mfe = min over every co-fold structure of E(structure, cut), and the structure it returns has that
    energy.  cofold_pf: FA and FB are the one-strand values (pinned above); FAB and FcAB against the enumeration weighted with
    exp(-E / kT) of the INTEGER evaluation (connected structures carry DuplexInit, halved for two equal strands).

    "distinct_sharp": no dangle-like entry lies where smooth() is curved, so the two loop models give every structure the same
    energy and EVERY pair must agree, to 1e-9 kcal/mol (rounding only): this is what pins the oracle's two-strand partition
    function under distinct tables, a non-zero MLbase, positive dangles and the probe's DuplexInit.  Under the other probes
    the models differ in the dangle-like terms (min(0, x) against smooth), by at most _clamp_smooth_gap() each, and a structure
    of n bases has at most n / 2 stems: |dF| <= gap * n / 2; how many pairs agree to 1e-6 there is printed."""
    pyoracle.build()
    orc = pyoracle.Oracle(PP.probe_blob(name))
    gap = _clamp_smooth_gap() / 100.0
    assert 0.015 < gap < 0.03
    cases = _cofold_cases()
    entered = connected = 0
    for s in cases:
        a, b = s.split("&")
        cut, flat = len(a), a + b
        dbs = cofold_structures(flat, cut)
        en = np.array([orc.eval_structure(flat, db, cut) for db in dbs])
        ss, e = orc.cofold_mfe(s)
        assert e == en.min() and orc.eval_structure(flat, ss.replace("&", ""), cut) == e, s
        w = np.exp(-en / 100.0 / KT)
        joined = np.array([any(i < cut <= j for i, j in _pairs_of(db)) for db in dbs])
        if a == b:
            w = np.where(joined, 0.5 * w, w)
        fa, fb, fcab, fab = orc.cofold_pf(s)
        assert abs(fa - orc.pf(a)) < 1e-9 and abs(fb - orc.pf(b)) < 1e-9, s
        F = -KT * np.log(w.sum())
        bound = 1e-9 if name == "distinct_sharp" else gap * len(flat) / 2
        assert abs(F - fab) <= bound, (s, F, fab)
        if joined.any():
            connected += 1
            Fc = -KT * np.log(w[joined].sum())
            assert abs(Fc - fcab) <= bound, (s, Fc, fcab)
        entered += abs(F - fab) < 1e-6
    print("%s: %d of %d pairs agree to 1e-6 kcal/mol, %d have a connected structure" % (name, entered, len(cases), connected))
    assert connected >= len(cases) // 2 and (name != "distinct_sharp" or entered == len(cases))
