"""Puzzle sets in lock-step with -nd on and an Edef term, host side: design.run_puzzle_batch(native_loop=False) on an oracle-backed
stand-in engine against design.run_design_fast of every puzzle alone.  The stand-in is test_puzzle_set_host.RaggedOracleEngine plus
the ensemble defect (one ragged call for the set, the rectangular call for a puzzle alone) and the second-best energy, all from
the CPU oracle, counted."""
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design
from desirna_amd import energy_scores as es
from tests.test_puzzle_set_host import HAIRPIN14, KEYS, RaggedOracleEngine, _input, _same_run, puzzles  # noqa: F401  (puzzles: fixture)

# (seed and step count chosen with the oracle: with -nd on every one of the three puzzles has, after the first exchange step, a
# solved replica whose second-best energy is not zero)
KW = dict(replicas=4, exchange=10, seed=5)
STEPS = 3
CASES = {"nd": dict(negative_design="on"), "edef": dict(scoring_f="Ed-Epf:0.5,Edef:5.0"),
         "both": dict(negative_design="on", scoring_f="Ed-Epf:0.5,Edef:5.0")}


class AuxOracleEngine(RaggedOracleEngine):
    def __init__(self, oracle):
        super().__init__(oracle)
        self.edef_ragged_sizes, self.edef_rect_calls, self.sub_calls, self.sub_folded = [], 0, 0, 0

    def ensemble_defect_ragged_arrays(self, flat_u8, lens, target_of):
        self.edef_ragged_sizes.append(len(lens))
        flat = bytes(np.asarray(flat_u8, dtype=np.uint8)).decode()
        offs = np.concatenate(([0], np.cumsum(lens)))
        return np.array([self.o.ensemble_defect(flat[offs[r]:offs[r + 1]], self.ragged_targets[int(target_of[r])])
                         for r in range(len(lens))], dtype=np.float64)

    def ensemble_defect_arrays(self, seqs_u8):
        self.edef_rect_calls += 1
        return np.array([self.o.ensemble_defect(bytes(r).decode(), self.targets[0]) for r in seqs_u8], dtype=np.float64)

    def subopt_energy(self, seqs):
        self.sub_calls += 1
        self.sub_folded += len(seqs)
        return np.array([self.o.subopt_energy(s) for s in seqs], dtype=np.int32)


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_with_aux_folds_equals_every_puzzle_alone(oracle, puzzles, case, monkeypatch):  # noqa: F811
    # more than one -sf term: the reference keeps the first only (parse_scoring_functions); all of them here
    monkeypatch.setattr(es, "parse_scoring_functions", lambda s, first_term_only=True, _p=es.parse_scoring_functions: _p(s, False))
    kw = dict(KW, **CASES[case])
    nd, edef = "negative_design" in kw, "Edef" in kw.get("scoring_f", "")
    eng = AuxOracleEngine(oracle)
    got = design.run_puzzle_batch(puzzles, steps=STEPS, native_loop=False, engine=eng, **kw)
    assert len(got) == len(puzzles)
    alone_folded = 0
    for inp, a in zip(puzzles, got):
        one = AuxOracleEngine(oracle)
        b = design.run_design_fast(inp, steps=STEPS, native_loop=False, engine=one, **kw)
        alone_folded += one.sub_folded
        _same_run(a, b)
        for col in ("subopt_e", "esubopt_minus_Epf", "mcc", "Epf", "edesired", "edesired_minus_Epf"):
            assert [r[col] for r in a["simulation_data"]] == [r[col] for r in b["simulation_data"]], col
        if nd:
            hits = [r for r in a["simulation_data"] if r["sim_step"] > 0 and r["mcc"] == 0 and r["subopt_e"] != 0]
            print(inp.name, case, "solved records with a second-best energy after step 0:", len(hits))
            assert hits, "the negative-design step never ran for %s: the case shows nothing" % inp.name
            assert all(r["esubopt_minus_Epf"] == r["subopt_e"] - r["Epf"] for r in hits)
            assert hasattr(a["best"], "subopt_e")
        else:
            assert all(r["subopt_e"] == 0 for r in a["simulation_data"]) and not hasattr(a["best"], "subopt_e")
        if edef and not nd:                                # the Edef term is in the score (the array state keeps no column of its own)
            assert all(0 < r["scoring_function"] - 0.5 * r["edesired_minus_Epf"] < 5 for r in a["simulation_data"])
    calls = 1 + STEPS * KW["exchange"]
    assert eng.ragged_calls == calls and eng.rect_calls == 0
    # the ensemble defect: one ragged call per scoring call, always with every chain, never the rectangular one
    assert eng.edef_ragged_sizes == ([len(puzzles) * KW["replicas"]] * calls if edef else []) and eng.edef_rect_calls == 0
    assert (one.edef_rect_calls > 0) == edef
    # the second-best folds: the same candidates as the runs alone
    assert eng.sub_folded == alone_folded and (eng.sub_calls > 0) == nd


def test_batch_still_refuses_what_it_cannot_run(puzzles):  # noqa: F811
    for bad in (_input("two", "((((....&....))))"), _input("pk", "((((..[[[..))))...]]]"),
                SimpleNamespace(**dict(vars(puzzles[0]), alt_sec_structs=[".(((......)))."]))):
        for kw in CASES.values():
            with pytest.raises(ValueError, match="still refused"):
                design.run_puzzle_batch([puzzles[0], bad], steps=1, engine=object(), **dict(KW, **kw))
    with pytest.raises(ValueError, match="-oa on"):
        design.run_puzzle_batch(puzzles, steps=1, engine=object(), oligo="on", **KW)
    # the routing test of --set is unchanged: -nd on and Edef sets still go to the per-puzzle driver
    assert design.batch_eligible(puzzles[0])
    assert not design.batch_eligible(puzzles[0], negative_design="on") and not design.batch_eligible(puzzles[0], oligo="on")
    assert not design.batch_eligible(puzzles[0], scoring_f="Edef:1.0") and not design.batch_eligible(puzzles[0], acgu={"A": 25})
