"""Sequence motifs (-motifs) on the GPU: the native Monte-Carlo loops, which take the motif set from the engine
(Engine.set_motifs), against the per-iteration loop, which adds HostKernels.motif_score to score_arrays -- bit for bit; the
lock-step loops against every puzzle alone; no motifs left in a shared engine; drna_set_motifs' argument errors.

Restraints and seeds were picked with the CPU oracle: an unpaired position holds no G (H), so the initial loops are UAAA...
and GNRA occurs when the closing stem ends in G; the records of every case hold sequences with and without the named motifs."""
import csv
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_puzzle_set_host import COUNTERS, KEYS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAIRPIN14 = "((((......))))"
MOTIFS = "GNRA,-2,GGGG,3,,0.5"          # the empty motif occurs everywhere: 0.5 is the term of a sequence without GNRA and GGGG
ACROSS = "UUCC"                          # two strands: fixed at the nick by the restraints (..UU&CC..), so it occurs only across it
KW = dict(replicas=4, exchange=6, steps=2)


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine as E
    e = E.Engine(max_R=16, max_L=40)
    yield e
    e.close()


def _inp(name, ss, restr=None):
    restr = restr or "".join("N" if c in "()" else "H" for c in ss)
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr=restr, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


@pytest.fixture(scope="module")
def puzzles():
    tg = {r["name"]: r["structure"] for r in csv.DictReader(open(os.path.join(GOLDEN, "eterna_v1_targets.csv")))}
    out = [_inp(n, tg[n], "N" * len(tg[n])) for n in ("eteV1_08.txt", "eteV1_03.txt")]
    assert [len(i.sec_struct) for i in out] == [12, 36]
    return out


def _terms(records, motifs):
    from desirna_amd import energy_scores as es
    opts = SimpleNamespace(motifs=es.parse_motifs(motifs))
    return [es.score_motifs(r["sequence"], opts) for r in records]


def _same_bits(a, b):
    """records (every column), counters and best of two runs: equal, the floats as doubles bit for bit"""
    ra, rb = a["simulation_data"], b["simulation_data"]
    assert len(ra) == len(rb) > 0
    worst = max(abs(x["scoring_function"] - y["scoring_function"]) for x, y in zip(ra, rb))
    print("largest difference of two scores:", worst)
    for x, y in zip(ra, rb):
        assert list(x) == list(y)
        for k in x:
            assert x[k] == y[k] and type(x[k]) is type(y[k]), (k, x[k], y[k], x["sequence"])
    for k in COUNTERS:
        assert a["stats"][k] == b["stats"][k], k
    assert vars(a["best"]) == vars(b["best"])
    assert a["steps"] == b["steps"] and a["solved"] == b["solved"] and a["temps"] == b["temps"]


@pytest.mark.parametrize("case", ["hairpin", "hairpin_nd", "hairpin_oa", "two_strands"])
def test_native_loop_equals_per_iteration_loop_with_motifs(eng, example_inputs, case):
    from desirna_amd import design
    if case == "two_strands":
        ss = example_inputs["RNA_RNA_complex_design_input"]["sec_struct"][0]
        cut = ss.index("&")
        assert (cut, len(ss) - cut - 1) == (17, 18)
        restr = "".join("N" if c in "()" else c if c == "&" else "H" for c in ss)
        inp = _inp(case, ss, restr[:cut - 2] + "UU&CC" + restr[cut + 3:])
        motifs, kw, bonus = MOTIFS + ",%s,1.25" % ACROSS, dict(KW, seed=2), "oligomer_bonus"
    else:
        inp, motifs, kw, bonus = _inp(case, HAIRPIN14), MOTIFS, dict(KW, seed=5), "monomer_bonus"
        kw.update({"hairpin_nd": dict(negative_design="on"), "hairpin_oa": dict(oligo="on")}.get(case, {}))
    nat = design.run_design_fast(inp, engine=eng, native_loop=True, motifs=motifs, **kw)
    assert eng.get_option("motifs") == motifs.count(",") // 2 + 1
    per = design.run_design_fast(inp, engine=eng, native_loop=False, motifs=motifs, **kw)
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    assert nat["stats"]["acc_mc"] > 0 and len(nat["simulation_data"]) == 4 * 3
    _same_bits(nat, per)
    # the term is in the score, last: -sf is Ed-Epf:1.0
    recs = nat["simulation_data"]
    terms = _terms(recs, motifs)
    for r, t in zip(recs, terms):
        assert r["scoring_function"] == ((r["edesired_minus_Epf"] - r["esubopt_minus_Epf"]) + r.get(bonus, 0.0)) + t, r
    # ... non-zero for the named motifs in some records and zero in others: otherwise the case shows nothing
    assert any(t == 0.5 for t in terms) and any(t != 0.5 for t in terms), sorted(set(terms))
    if case == "two_strands":
        assert all(ACROSS in r["sequence"].replace("&", "") and ACROSS not in r["sequence"].replace("&", " ") for r in recs)
        assert all(t in (0.5, -1.5, 3.5, 1.5) for t in terms), sorted(set(terms))          # never + 1.25: no match across the nick
        assert all("oligomer_bonus" in r for r in recs)
    if case == "hairpin_nd":
        assert any(r["mcc"] == 0 and r["esubopt_minus_Epf"] != 0 for r in recs)
    if case == "hairpin_oa":
        assert all(r["monomer_bonus"] > 0 for r in recs)


@pytest.mark.parametrize("nd", ["off", "on"])
def test_lock_step_loops_equal_every_puzzle_alone_with_motifs(eng, puzzles, nd):
    from desirna_amd import design
    kw = dict(KW, seed=5, engine=eng, motifs=MOTIFS, negative_design=nd)
    got = design.run_puzzle_batch(puzzles, **kw)
    assert eng.get_option("motifs") == 3
    terms = []
    for inp, a in zip(puzzles, got):
        b = design.run_design_fast(inp, **kw)
        assert a["used_native_loop"] is True and b["used_native_loop"] is True
        assert len(a["simulation_data"]) == len(b["simulation_data"]) == 4 * 3
        for k in KEYS + (("subopt_e",) if nd == "on" else ()):
            assert [r[k] for r in a["simulation_data"]] == [r[k] for r in b["simulation_data"]], (inp.name, k)
        for k in COUNTERS:
            assert a["stats"][k] == b["stats"][k], (inp.name, k)
        assert vars(a["best"]) == vars(b["best"]) and a["steps"] == b["steps"] and a["solved"] == b["solved"]
        ts = _terms(a["simulation_data"], MOTIFS)
        for r, t in zip(a["simulation_data"], ts):
            assert r["scoring_function"] == (r["edesired_minus_Epf"] - r["esubopt_minus_Epf"]) + t
        terms += ts
    assert len(set(terms)) > 1, terms          # (the same set for both puzzles, and it told sequences apart)


def test_a_shared_engine_carries_no_motifs_into_the_next_run(eng, puzzles):
    from desirna_amd import design, engine as E
    inp, kw = _inp("hairpin", HAIRPIN14), dict(KW, seed=5)
    with_motifs = design.run_design_fast(inp, engine=eng, motifs=MOTIFS, **kw)
    assert eng.get_option("motifs") == 3
    after = design.run_design_fast(inp, engine=eng, **kw)
    assert eng.get_option("motifs") == 0 and after["used_native_loop"] is True
    fresh = E.Engine(max_R=4, max_L=14)
    try:
        assert fresh.get_option("motifs") == 0
        want = design.run_design_fast(inp, engine=fresh, **kw)
    finally:
        fresh.close()
    _same_bits(after, want)
    assert [r["scoring_function"] for r in after["simulation_data"]] != [r["scoring_function"] for r in with_motifs["simulation_data"]]
    assert all(r["scoring_function"] == r["edesired_minus_Epf"] for r in after["simulation_data"])
    # the lock-step driver clears the set, too
    eng.set_motifs({"GGGG": 3.0})
    assert eng.get_option("motifs") == 1
    design.run_puzzle_batch(puzzles[:1], engine=eng, **kw)
    assert eng.get_option("motifs") == 0


def test_set_motifs_argument_errors_leave_the_set_as_it_was(eng):
    from desirna_amd import engine as E
    eng.set_motifs([("GNRA", -2.0), ("GGGG", 3.0)])
    assert eng.get_option("motifs") == 2
    for bad in ([("GGGG", 1.0), ("GNXA", 1.0)], {"gnra": 1.0}, [("G&C", 1.0)]):
        with pytest.raises(E.EngineError) as err:
            eng.set_motifs(bad)
        assert err.value.code == -1 and "drna_set_motifs" in str(err.value)
        assert eng.get_option("motifs") == 2
    with pytest.raises(E.EngineError):
        eng.set_option("motifs", 1)                       # read-only
    eng.set_motifs([("GNRA", -2.0), ("GNRA", 1.0)])       # one key
    assert eng.get_option("motifs") == 1
    eng.set_motifs(None)
    assert eng.get_option("motifs") == 0
