"""Negative design (-nd on) on the host path, no GPU: run_design (energy_scores.ReplicaScorer, the reference's order of additions)
against run_design_fast(negative_design="on", native_loop=False), both on oracle-backed stand-in engines that count their
second-best calls.  The oracle has a one-strand second-best energy; for two strands the stand-in derives one from the co-fold
MFE and the sequence (the drivers only transport the value, the kernels that compute it have their own tests).

Second-best calls / solved candidates they covered in the runs below, as observed when the seeds were picked (each driver):
hairpin14 61 / 322, standard36 241 / 1449, homodimer 81 / 429; with "off": 0."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design
from desirna_amd import energy_scores as es
from tests.test_cofold_native_host import OracleCoEngine
from tests.test_design_driver import OracleEngine

HAIRPIN14 = "((((......))))"


class NdEngine(OracleEngine):
    """one strand: + subopt_energy"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.calls = self.folded = 0

    def subopt_energy(self, seqs):
        self.calls += 1
        self.folded += len(seqs)
        return np.array([self.o.subopt_energy(s) for s in seqs], dtype=np.int32)


class NdCoEngine(OracleCoEngine):
    """two strands: + cofold_subopt_energy, a fixed function of the pair (co-fold MFE + 0.1 .. 4 kcal/mol)"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.calls = self.folded = 0

    def cofold_subopt_energy(self, seqs):
        self.calls += 1
        self.folded += len(seqs)
        return np.array([self.o.cofold_mfe(s)[1] + 10 * (1 + zlib.crc32(s.encode()) % 40) for s in seqs], dtype=np.int32)


def _inp(name, ss, restr):
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr=restr, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


def _case(example_inputs, which):
    if which == "hairpin14":
        return _inp(which, HAIRPIN14, "N" * 14), "off", dict(replicas=6, exchange=15, steps=4, seed=9)
    if which == "standard36":
        ex = example_inputs["Standard_design_input"]
        return _inp(which, ex["sec_struct"][0], ex["seq_restr"][0]), "off", dict(replicas=8, exchange=40, steps=6, seed=3)
    ex = example_inputs["Homodimer_design_input"]
    return _inp(which, ex["sec_struct"][0], ex["seq_restr"][0]), "on", dict(replicas=6, exchange=20, steps=4, seed=9)


def _run_both(oracle, inp, dimer, kw, nd):
    two = "&" in inp.sec_struct
    mk = NdCoEngine if two else NdEngine
    ea, eb = mk(oracle), mk(oracle)
    state = ("homodimer" if dimer == "on" else "heterodimer") if two else "none"
    opts = SimpleNamespace(oligo_state=state, pks="off", subopt=nd, motifs=None, param="1999",
                           scoring_f=es.parse_scoring_functions("Ed-Epf:1.0"))
    a = design.run_design(inp, scorer=es.ReplicaScorer(inp, opts, kw["replicas"], engine=ea), dimer=dimer, subopt=nd, **kw)
    b = design.run_design_fast(inp, engine=eb, native_loop=False, dimer=dimer, negative_design=nd, **kw)
    assert not b["used_native_loop"]
    return a, b, ea, eb


def _same_walk(a, b):
    ra, rb = a["simulation_data"], b["simulation_data"]
    assert [r["sequence"] for r in ra] == [r["sequence"] for r in rb]
    assert [r["mfe_ss"] for r in ra] == [r["mfe_ss"] for r in rb]
    assert [r["temp_shelf"] for r in ra] == [r["temp_shelf"] for r in rb]
    for x, y in zip(ra, rb):
        assert abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
        assert x["subopt_e"] == y["subopt_e"]
        assert abs(x["esubopt_minus_Epf"] - y["esubopt_minus_Epf"]) < 1e-9
    for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
        assert a["stats"][k] == b["stats"][k], k
    assert a["best"].sequence == b["best"].sequence and a["best"].mfe_ss == b["best"].mfe_ss
    assert abs(a["best"].scoring_function - b["best"].scoring_function) < 1e-9
    assert a["best"].subopt_e == getattr(b["best"], "subopt_e", 0)          # (with "off" the fast driver's best has no such field)


@pytest.mark.parametrize("which", ["hairpin14", "standard36", "homodimer"])
def test_both_drivers_walk_the_same_trajectory_with_nd_on(oracle, example_inputs, which):
    inp, dimer, kw = _case(example_inputs, which)
    a, b, ea, eb = _run_both(oracle, inp, dimer, kw, "on")
    _same_walk(a, b)
    print(which, "second-best calls / folds:", ea.calls, ea.folded, eb.calls, eb.folded)
    assert ea.calls >= 1 and (ea.calls, ea.folded) == (eb.calls, eb.folded)        # a solved candidate took the branch
    assert any(r["mcc"] == 0 and r["esubopt_minus_Epf"] != 0 for r in b["simulation_data"])


@pytest.mark.parametrize("which", ["hairpin14", "homodimer"])
def test_nd_off_makes_no_second_best_call_and_keeps_the_trajectory(oracle, example_inputs, which):
    inp, dimer, kw = _case(example_inputs, which)
    a, b, ea, eb = _run_both(oracle, inp, dimer, kw, "off")
    assert ea.calls == 0 and eb.calls == 0
    _same_walk(a, b)
    c = design.run_design_fast(inp, engine=type(eb)(oracle), native_loop=False, dimer=dimer, **kw)      # the keyword left out: today's call
    assert [r["sequence"] for r in c["simulation_data"]] == [r["sequence"] for r in b["simulation_data"]]
    assert [r["scoring_function"] for r in c["simulation_data"]] == [r["scoring_function"] for r in b["simulation_data"]]
    assert all(r["subopt_e"] == 0 and r["esubopt_minus_Epf"] == 0 for r in b["simulation_data"])
    assert not hasattr(c["best"], "subopt_e")


def test_two_strands_nd_term_before_the_bonus(oracle, example_inputs):
    """a solved homodimer record with both terms non-zero: score = ((Ed - Epf) - (subopt_e - Epf)) + bonus, in that order"""
    inp, dimer, kw = _case(example_inputs, "homodimer")
    a, b, ea, eb = _run_both(oracle, inp, dimer, kw, "on")
    hits = [r for r in b["simulation_data"] if r["mcc"] == 0 and r["esubopt_minus_Epf"] != 0 and r["oligomer_bonus"] != 0]
    assert hits
    for r in hits:
        want = (r["edesired_minus_Epf"] - r["esubopt_minus_Epf"]) + r["oligomer_bonus"]
        assert r["scoring_function"] == want
