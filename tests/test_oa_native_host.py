"""Avoid oligomerization (-oa on) on the host path, no GPU: run_design (energy_scores.ReplicaScorer, which folds s & s through
cofold_batch and adds the monomer-fraction term itself) against run_design_fast(oligo="on", native_loop=False), which takes the
term from score_arrays(self_dimer=True) / Engine.self_dimer.  Both on oracle-backed stand-in engines that count their self-dimer
folds; the kernel that computes them on the GPU has its own tests."""
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design
from desirna_amd import energy_scores as es
from tests.test_nd_native_host import HAIRPIN14, NdEngine

_F4 = {}            # oracle.cofold_pf(s & s) by sequence: both drivers fold the same candidates


class OaEngine(NdEngine):
    """one strand: + the self-dimer, as cofold_batch([s & s], NEED_PF) (ReplicaScorer's dimer engine) and as self_dimer(seqs)"""
    max_L = 1 << 20                                 # (ReplicaScorer opens no second engine)

    def __init__(self, oracle):
        super().__init__(oracle)
        self.dimer_calls = self.dimer_folds = 0

    def _f4(self, seqs):
        self.dimer_calls += 1
        self.dimer_folds += len(seqs)
        for s in seqs:
            if s not in _F4:
                _F4[s] = self.o.cofold_pf(s + "&" + s)
        return np.array([_F4[s] for s in seqs])

    def cofold_batch(self, seqs, flags=0):
        assert all(s.split("&")[0] == s.split("&")[1] for s in seqs)
        F = self._f4([s.split("&")[0] for s in seqs])
        return {"FA": F[:, 0], "FB": F[:, 1], "FcAB": F[:, 2], "FAB": F[:, 3]}

    def self_dimer(self, seqs):
        F = self._f4(seqs)
        return {"FA": F[:, 0], "FcAA": F[:, 2], "FAA": F[:, 3],
                "oligo_fraction": np.array([float(es.oligo_fraction(f[0], f[1], f[2])) for f in F])}


def _inp(name, ss, restr):
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr=restr, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


def _case(example_inputs, which):
    if which == "hairpin14":
        return _inp(which, HAIRPIN14, "N" * 14), dict(replicas=6, exchange=15, steps=4, seed=9)
    ex = example_inputs["Standard_design_input"]
    return _inp(which, ex["sec_struct"][0], ex["seq_restr"][0]), dict(replicas=8, exchange=40, steps=6, seed=3)


def _run_both(oracle, inp, kw, oligo, nd="off"):
    ea, eb = OaEngine(oracle), OaEngine(oracle)
    opts = SimpleNamespace(oligo_state="avoid" if oligo == "on" else "none", pks="off", subopt=nd, motifs=None, param="1999",
                           scoring_f=es.parse_scoring_functions("Ed-Epf:1.0"))
    a = design.run_design(inp, scorer=es.ReplicaScorer(inp, opts, kw["replicas"], engine=ea), oligo=oligo, subopt=nd, **kw)
    b = design.run_design_fast(inp, engine=eb, native_loop=False, oligo=oligo, negative_design=nd, **kw)
    assert not b["used_native_loop"]
    return a, b, ea, eb


def _same_walk(a, b, oa=True):
    ra, rb = a["simulation_data"], b["simulation_data"]
    assert len(ra) == len(rb) > 0
    assert [r["sequence"] for r in ra] == [r["sequence"] for r in rb]
    assert [r["mfe_ss"] for r in ra] == [r["mfe_ss"] for r in rb]
    assert [r["temp_shelf"] for r in ra] == [r["temp_shelf"] for r in rb]
    for x, y in zip(ra, rb):
        assert abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
        assert x["subopt_e"] == y["subopt_e"]
        if oa:
            assert abs(x["oligo_fraction"] - y["oligo_fraction"]) < 1e-9 and abs(x["monomer_bonus"] - y["monomer_bonus"]) < 1e-9
            assert list(x) == list(y)                      # the same columns in the same order: the CSV schema
    for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
        assert a["stats"][k] == b["stats"][k], k
    assert a["best"].sequence == b["best"].sequence and a["best"].mfe_ss == b["best"].mfe_ss
    assert abs(a["best"].scoring_function - b["best"].scoring_function) < 1e-9
    if oa:
        assert abs(a["best"].oligo_fraction - b["best"].oligo_fraction) < 1e-9
        assert abs(a["best"].monomer_bonus - b["best"].monomer_bonus) < 1e-9


@pytest.mark.parametrize("which", ["hairpin14", "standard36"])
@pytest.mark.parametrize("nd", ["off", "on"])
def test_both_drivers_walk_the_same_trajectory_with_oa_on(oracle, example_inputs, which, nd):
    inp, kw = _case(example_inputs, which)
    a, b, ea, eb = _run_both(oracle, inp, kw, "on", nd)
    _same_walk(a, b)
    assert (ea.dimer_calls, ea.dimer_folds) == (eb.dimer_calls, eb.dimer_folds)
    assert ea.dimer_folds == kw["replicas"] * (1 + kw["exchange"] * kw["steps"])          # every candidate, and the start
    rb = b["simulation_data"]
    assert all(0 < r["oligo_fraction"] < 1 and r["monomer_bonus"] > 0 for r in rb)
    if nd == "on":
        assert ea.calls >= 1 and (ea.calls, ea.folded) == (eb.calls, eb.folded)
        hits = [r for r in rb if r["mcc"] == 0 and r["esubopt_minus_Epf"] != 0]
        assert hits                                        # the bonus is the last addition, after the negative-design term
        for r in hits:
            assert r["scoring_function"] == (r["edesired_minus_Epf"] - r["esubopt_minus_Epf"]) + r["monomer_bonus"]
    else:
        assert all(r["scoring_function"] == r["edesired_minus_Epf"] + r["monomer_bonus"] for r in rb)


def test_oa_off_makes_no_self_dimer_call_and_keeps_the_trajectory(oracle, example_inputs):
    inp, kw = _case(example_inputs, "hairpin14")
    a, b, ea, eb = _run_both(oracle, inp, kw, "off")
    assert ea.dimer_calls == 0 and eb.dimer_calls == 0
    _same_walk(a, b, oa=False)
    c = design.run_design_fast(inp, engine=OaEngine(oracle), native_loop=False, **kw)          # the keyword left out: today's call
    assert [(r["sequence"], r["scoring_function"]) for r in c["simulation_data"]] == \
        [(r["sequence"], r["scoring_function"]) for r in b["simulation_data"]]
    assert all("oligo_fraction" not in r and "monomer_bonus" not in r for r in b["simulation_data"])
    assert not hasattr(c["best"], "oligo_fraction")


def test_score_arrays_default_leaves_the_bonus_to_the_replica_scorer(oracle):
    """score_arrays(self_dimer=False) with oligo_state "avoid" adds nothing (ReplicaScorer.score adds the term itself: a default-on
    would count it twice in run_design); with two strands the switch changes nothing"""
    from desirna_amd import engine as E
    eng = OaEngine(oracle)
    eng.set_targets([HAIRPIN14])
    seqs = np.frombuffer(b"GGGGAAAAAACCCC" + b"GCGCAAAAAAGCGC", dtype=np.uint8).reshape(2, 14)
    hk, sf = E.HostKernels(), es.parse_scoring_functions("Ed-Epf:1.0")
    off = es.score_arrays(eng, hk, HAIRPIN14, sf, seqs, "avoid")
    assert eng.dimer_calls == 0 and off.oligo_fraction is None and off.bonus is None
    on = es.score_arrays(eng, hk, HAIRPIN14, sf, seqs, "avoid", self_dimer=True)
    assert eng.dimer_calls == 1 and np.array_equal(on.score, off.score + on.bonus)
    none = es.score_arrays(eng, hk, HAIRPIN14, sf, seqs, "none", self_dimer=True)
    assert eng.dimer_calls == 1 and none.bonus is None and np.array_equal(none.score, off.score)
    rec = es.record(on, 1)
    assert rec.oligo_fraction == on.oligo_fraction[1] and rec.monomer_bonus == on.bonus[1] and not hasattr(rec, "oligomer_bonus")


def test_cli_routes_oa_on_to_the_fast_driver(monkeypatch, tmp_path):
    """-oa on alone no longer forces the Python host; -acgu on still does"""
    f = tmp_path / "d.txt"
    f.write_text(">name\nx\n>seq_restr\n%s\n>sec_struct\n%s\n" % ("N" * 14, HAIRPIN14))
    seen = []

    def fake(which):
        def run(inp, **kw):
            seen.append((which, kw.get("oligo")))
            best = SimpleNamespace(sequence="A" * 14, mfe_ss="." * 14, Epf=0.0, edesired=0.0, mcc=1.0, scoring_function=0.0)
            return {"best": best, "solved": False, "steps": 0, "stats": {"scored": 0, "elapsed_s": 0.0}}
        return run

    monkeypatch.setattr(design, "run_design", fake("python"))
    monkeypatch.setattr(design, "run_design_fast", fake("fast"))
    design.main(["-f", str(f), "-oa", "on"])
    design.main(["-f", str(f), "-oa", "on", "-acgu", "on", "-acgu_content", "25,25,25,25"])
    design.main(["-f", str(f), "-oa", "on", "--python-host"])
    design.main(["-f", str(f)])
    assert seen == [("fast", "on"), ("python", "on"), ("python", "on"), ("fast", None)]
