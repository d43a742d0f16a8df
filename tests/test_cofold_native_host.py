"""Two-strand designs on the native host path (no GPU): drna_propose_batch_co against DesignProblem.mutation_position + mutate,
draw for draw, and run_design_fast's per-iteration two-strand loop against run_design, both scored by the CPU oracle."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design, engine
from desirna_amd import energy_scores as es
from desirna_amd.sim_score import batch_metrics

# a homodimer whose two sub-structures differ: '((((....&....))))' with a one-nucleotide bulge in the first strand
BULGED = "((.((....&....))))"
EQUAL = ".((((....)))).&.((((....))))."          # two equal sub-structures (a hairpin per strand)


@pytest.fixture(scope="module")
def hk():
    return engine.HostKernels()


def _cases(example_inputs):
    het = example_inputs["RNA_RNA_complex_design_input"]
    hom = example_inputs["Homodimer_design_input"]
    return [("heterodimer", het["sec_struct"][0], het["seq_restr"][0]),
            ("homodimer", hom["sec_struct"][0], hom["seq_restr"][0]),
            ("homodimer", BULGED, "NNNNNNNNN&NNNNNNNN"),
            ("homodimer", EQUAL, "N" * 14 + "&" + "N" * 14),
            ("heterodimer", BULGED, "NNGNNNNAN&NNNNNUNN")]          # IUPAC-fixed positions, one of them paired


def _random_structure(rng, target, n_flip):
    """a balanced structure near the target: n_flip of its pairs opened (what an MFE structure of a poor sequence looks like)"""
    pt = design.pair_table(target)
    pairs = [(i, int(p)) for i, p in enumerate(pt) if p > i]
    s = list(target)
    for i, j in rng.sample(pairs, min(n_flip, len(pairs))):
        s[i] = s[j] = "."
    return "".join(s)


@pytest.mark.parametrize("targeted", [False, True])
def test_proposer_parity_draw_for_draw(hk, example_inputs, targeted):
    """8 replicas x 200 consecutive proposals: identical strings and identical streams afterwards, on every shelf of a
    4-shelf ladder, with targeted moves on and off."""
    R, n_shelves, tm_max, tm_min = 8, 4, 0.7, 0.0
    for state, tg, restr in _cases(example_inputs):
        prob = design.DesignProblem(tg, restr)
        assert prob.two_strands
        amp = tg.index("&")
        rngs = [random.Random(r) for r in range(R)]
        st = hk.rng_seed(np.arange(R))
        aux = random.Random(77)
        cur = [prob.initial_sequence(random.Random(5))] * R
        if state == "homodimer" and tg.split("&")[0] == tg.split("&")[1]:
            a = cur[0].split("&")[0]
            cur = [a + "&" + a] * R
        shelves = np.array([r % n_shelves for r in range(R)], dtype=np.int32)
        for it in range(200):
            ss = [_random_structure(aux, tg, aux.randrange(0, 4)) for _ in range(R)]
            want = []
            for r in range(R):
                pos = prob.mutation_position(ss[r], int(shelves[r]), n_shelves, tm_max, tm_min, targeted, rngs[r])
                want.append(prob.mutate(cur[r], pos, rngs[r], state))
            got = hk.propose_co(prob, state, np.frombuffer("".join(cur).encode(), np.uint8).reshape(R, -1),
                                np.frombuffer("".join(ss).encode(), np.uint8).reshape(R, -1), shelves, n_shelves, tm_max, tm_min,
                                targeted, st)
            got = [bytes(g).decode() for g in got]
            assert got == want, (state, tg, it)
            for g in got:                                          # untouched columns and symmetry
                assert g[amp] == "&" and g.count("&") == 1
                assert all(g[i] == c for i, c in enumerate(restr) if c in "ACGU")
                if state == "homodimer" and tg.split("&")[0] == tg.split("&")[1]:
                    assert g.split("&")[0] == g.split("&")[1]
            cur = want
        assert list(hk.rng_random(st)) == [g.random() for g in rngs], (state, tg)


def test_targeted_move_on_the_nick_changes_nothing(hk):
    """every pair of the current structure is a false positive next to the '&': with probability 1 the move lands in the
    window, which holds the '&' column; there nothing changes, after the same draws as in Python"""
    tg = "....&...."
    prob = design.DesignProblem(tg, "NNNN&NNNN")
    ss = "...(&)..."
    R = 8
    rngs = [random.Random(r) for r in range(R)]
    st = hk.rng_seed(np.arange(R))
    cur = ["ACGU&UGCA"] * R
    hit = 0
    for _ in range(60):
        want = []
        for r in range(R):
            pos = prob.mutation_position(ss, 0, 4, 1.0, 1.0, True, rngs[r])
            hit += pos == 4
            want.append(prob.mutate(cur[r], pos, rngs[r], "heterodimer"))
        got = hk.propose_co(prob, "heterodimer", np.frombuffer("".join(cur).encode(), np.uint8).reshape(R, -1),
                            np.frombuffer((ss * R).encode(), np.uint8).reshape(R, -1), np.zeros(R, np.int32), 4, 1.0, 1.0, True, st)
        assert [bytes(g).decode() for g in got] == want
        cur = want
    assert hit > 0
    assert list(hk.rng_random(st)) == [g.random() for g in rngs]


class OracleCoScorer:
    """ReplicaScorer._score_two_strands with the numbers of the CPU oracle (tests only)"""

    def __init__(self, oracle, target, scoring_f, oligo_state):
        self.o, self.target, self.sf, self.state = oracle, target, scoring_f, oligo_state

    def score(self, seqs):
        ss1, ss2 = self.target.split("&")
        out = []
        for s in seqs:
            ss, emfe = self.o.cofold_mfe(s)
            fa, fb, fcab, fab = self.o.cofold_pf(s)
            sc = es.ScoreSeq(s)
            sc.get_Epf(fab)
            sc.get_mfe_ss(ss)
            sc.get_edesired(self.o.eval_structure(s, self.target, len(ss1)) / 100.0)
            sc.get_edesired_minus_Epf(sc.Epf, sc.edesired)
            mcc, rec, prec = batch_metrics(self.target.replace("&", "Ee"), [ss.replace("&", "Ee")])[0]
            sc.get_precision(prec); sc.get_recall(rec); sc.get_mcc(mcc)
            sc.get_scoring_function(self.sf)
            sc.oligo_fraction = float(es.oligo_fraction(fa, fb, fcab))
            if self.state == "heterodimer" or ss1 != ss2:
                sc.oligomer_bonus = float(es.kTlog_oligo_fraction(sc.oligo_fraction))
            else:
                sc.oligomer_bonus = float(es.kTlog_monomer_fraction(sc.oligo_fraction))
            sc.scoring_function = sc.scoring_function + sc.oligomer_bonus
            out.append(sc)
        return out


class OracleCoEngine:
    """Duck-typed stand-in for engine.Engine in run_design_fast's per-iteration two-strand loop (tests only)"""
    TERM_IDS = {}

    def __init__(self, oracle):
        self.o, self.targets = oracle, []

    def set_targets(self, targets):
        self.targets = list(targets)

    def cofold_batch(self, seqs, flags=0):
        cut = seqs[0].index("&")
        ss, em, F, Ed = [], [], [], []
        for s in seqs:
            a, b = self.o.cofold_mfe(s)
            ss.append(a); em.append(b)
            F.append(self.o.cofold_pf(s))
            Ed.append([self.o.eval_structure(s, self.targets[0], cut)])
        F = np.array(F)
        return {"Emfe": np.array(em, dtype=np.int32), "Ed": np.array(Ed, dtype=np.int32), "mfe_ss": ss, "FA": F[:, 0], "FB": F[:, 1],
                "FcAB": F[:, 2], "FAB": F[:, 3]}


@pytest.mark.parametrize("run,dimer", [("RNA_RNA_complex_design_input", "off"), ("Homodimer_design_input", "on")])
def test_fast_two_strand_driver_equals_python_driver_with_oracle(oracle, example_inputs, run, dimer):
    ex = example_inputs[run]
    inp = SimpleNamespace(name=run, sec_struct=ex["sec_struct"][0], seq_restr=ex["seq_restr"][0], seed_seq=None, alt_sec_struct=None,
                          alt_sec_structs=None)
    sf = es.parse_scoring_functions("Ed-Epf:1.0")
    sc = OracleCoScorer(oracle, inp.sec_struct, sf, "homodimer" if dimer == "on" else "heterodimer")
    a = design.run_design(inp, replicas=6, exchange=15, steps=4, seed=9, scorer=sc, dimer=dimer)
    b = design.run_design_fast(inp, replicas=6, exchange=15, steps=4, seed=9, engine=OracleCoEngine(oracle), native_loop=False,
                               dimer=dimer)
    assert not b["used_native_loop"]
    ra, rb = a["simulation_data"], b["simulation_data"]
    assert [r["sequence"] for r in ra] == [r["sequence"] for r in rb]
    assert [r["temp_shelf"] for r in ra] == [r["temp_shelf"] for r in rb]
    assert [r["mfe_ss"] for r in ra] == [r["mfe_ss"] for r in rb]
    assert all("&" in r["sequence"] and "&" in r["mfe_ss"] for r in rb)
    for x, y in zip(ra, rb):
        assert abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
        assert abs(x["oligo_fraction"] - y["oligo_fraction"]) < 1e-9 and abs(x["oligomer_bonus"] - y["oligomer_bonus"]) < 1e-9
    for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
        assert a["stats"][k] == b["stats"][k], k
    assert a["best"].sequence == b["best"].sequence and abs(a["best"].scoring_function - b["best"].scoring_function) < 1e-9


def test_two_strands_with_alternative_structures_still_raise(example_inputs):
    ex = example_inputs["RNA_RNA_complex_design_input"]
    tg = ex["sec_struct"][0]
    inp = SimpleNamespace(name="x", sec_struct=tg, seq_restr=ex["seq_restr"][0], seed_seq=None, alt_sec_struct=tg,
                          alt_sec_structs=[tg])
    with pytest.raises(NotImplementedError):
        design.run_design_fast(inp, replicas=2, exchange=1, steps=1, engine=OracleCoEngine(None), native_loop=False)
