"""The auxiliary folds of a ragged batch on the GPU: drna_ensemble_defect_ragged and drna_subopt_energy_ragged against the uniform
calls per length (byte for byte, both kernel classes, through several workspace chunks) and against the CPU emulation of the
kernels; drna_mc_run_ragged_nd against drna_mc_run_nd of every puzzle alone (bit for bit); the batch driver with -nd on and an
Edef term on the native loop against run_design_fast per puzzle; the argument errors of the three symbols; the state they leave."""
import csv
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_puzzle_set_host import COUNTERS, KEYS, _input

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the lengths sit on both sides of both host bounds: EDEF_LDS_HOST_MAX = 40 (40 | 42), SUB_LDS_MAX = 79 (75 | 80); 202 nt is the
# engine's longest
BY_LEN = {12: "eteV1_08", 36: "eteV1_03", 40: "eteV1_65", 42: "eteV1_20", 75: "eteV1_75", 80: "eteV1_52", 105: "eteV1_16",
          202: "eteV1_98"}
PER_LEN = (2, 3, 4, 2, 3, 4, 2, 3)                    # sequences per length: the golden solution, then random ones
MC_LENS = (12, 36, 42, 80, 105)
MC_R, N_ITER = 4, 12
MAX_R = max(sum(PER_LEN), MC_R * len(MC_LENS))


def _rand(rng, n):
    return "".join(rng.choice(list("ACGU"), size=n))


@pytest.fixture(scope="module")
def gold():
    rows = csv.DictReader(open(os.path.join(GOLDEN, "eterna_v1_solutions.csv")))
    sol = {r["name"].replace(".txt", ""): (r["sequence"], r["structure"]) for r in rows}
    out = {n: sol[name] for n, name in BY_LEN.items()}
    assert all(len(s) == n == len(t) for n, (s, t) in out.items())
    return out


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine as E
    e = E.Engine(max_R=MAX_R, max_L=202)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(gold):
    """two to four sequences per length in shuffled caller order: sequences, their structure's index, the structures"""
    rng = np.random.default_rng(77)
    lens = sorted(gold)
    rows = [(n, gold[n][0] if k == 0 else _rand(rng, n)) for n, cnt in zip(lens, PER_LEN) for k in range(cnt)]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    return SimpleNamespace(seqs=[s for _, s in rows], tof=[lens.index(n) for n, _ in rows], structs=[gold[n][1] for n in lens], lens=lens)


def _uniform_reference(eng, batch):
    """per length: ensemble_defect after set_targets, subopt_energy(want_both) -> arrays in the batch's order"""
    R = len(batch.seqs)
    ed, E2, E12 = np.zeros(R), np.zeros(R, np.int32), np.zeros((R, 2), np.int32)
    for t, n in enumerate(batch.lens):
        rows = [r for r in range(R) if batch.tof[r] == t]
        eng.set_targets([batch.structs[t]])
        ed[rows] = eng.ensemble_defect([batch.seqs[r] for r in rows])
        a, b = eng.subopt_energy([batch.seqs[r] for r in rows], want_both=True)
        E2[rows], E12[rows] = a, b
    return ed, E2, E12


@pytest.mark.parametrize("lds", [1, 0], ids=["lds", "general"])
def test_ragged_entry_points_equal_the_uniform_calls(eng, batch, lds):
    eng.set_option("edef_lds", lds)
    eng.set_option("subopt_lds", lds)
    try:
        eng.set_targets_ragged(batch.structs)
        c0 = eng.get_option("edef_lds_calls")
        ed = eng.ensemble_defect_ragged(batch.seqs, batch.tof)
        # 12, 36 and 40 nt share ONE launch of the fused kernel
        assert eng.get_option("edef_lds_calls") - c0 == lds
        t = eng.last_edef_timing()
        assert t["inside"] > 0 and t["outside"] > 0          # the sums over the launches (42 nt and longer: two kernels)
        E2, E12 = eng.subopt_energy_ragged(batch.seqs, want_both=True)
        E2_only = eng.subopt_energy_ragged(batch.seqs)
        want_ed, want_E2, want_E12 = _uniform_reference(eng, batch)
    finally:
        eng.set_option("edef_lds", 1)
        eng.set_option("subopt_lds", 1)
    for r, s in enumerate(batch.seqs):
        assert ed[r:r + 1].tobytes() == want_ed[r:r + 1].tobytes(), (len(s), ed[r], want_ed[r])
        assert E2[r] == want_E2[r] == E2_only[r] and E12[r].tobytes() == want_E12[r].tobytes(), (len(s), E12[r], want_E12[r])
    assert (ed > 0).all() and (ed < 1).all() and (E12[:, 0] <= E12[:, 1]).all()


def test_ragged_entry_points_through_several_chunks(eng, batch, monkeypatch):
    """a workspace of a few slots (and another pitch: max_L = 400): the general classes of the ensemble defect go through several
    chunks and return the same bytes; the second-best call refuses a batch above the slots, as the uniform call does"""
    from desirna_amd import engine as E
    eng.set_targets_ragged(batch.structs)
    monkeypatch.setenv("DRNA_WS_GB", "0.1")
    small = E.Engine(max_R=len(batch.seqs), max_L=400, device=0)
    try:
        slots = small.get_option("workspace_slots")
        n_general = sum(len(s) > 40 for s in batch.seqs)
        assert 4 <= slots < n_general, (slots, n_general)                   # two chunks at least with edef_lds on, more without
        small.set_targets_ragged(batch.structs)
        for lds in (1, 0):
            eng.set_option("edef_lds", lds)
            small.set_option("edef_lds", lds)
            c0 = small.get_option("edef_lds_calls")
            a, b = eng.ensemble_defect_ragged(batch.seqs, batch.tof), small.ensemble_defect_ragged(batch.seqs, batch.tof)
            assert small.get_option("edef_lds_calls") - c0 == lds
            assert a.tobytes() == b.tobytes(), lds
        with pytest.raises(E.EngineError) as err:
            small.subopt_energy_ragged(batch.seqs)
        assert err.value.code == -1 and "workspace" in str(err.value)
        few = batch.seqs[:slots]
        x, y = eng.subopt_energy_ragged(few, want_both=True), small.subopt_energy_ragged(few, want_both=True)
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
        # a bad letter in a later chunk is named by the caller's index
        order = sorted(range(len(batch.seqs)), key=lambda r: -len(batch.seqs[r]))
        r_bad = order[slots + 1]
        seqs = list(batch.seqs)
        seqs[r_bad] = seqs[r_bad][:5] + "X" + seqs[r_bad][6:]
        with pytest.raises(E.EngineError) as err:
            small.ensemble_defect_ragged(seqs, batch.tof)
        assert err.value.code == -4 and "sequence %d " % r_bad in str(err.value), str(err.value)
    finally:
        eng.set_option("edef_lds", 1)
        small.close()


def test_ragged_entry_points_against_the_emulated_kernels(eng, gold):
    """One ragged call of 12, 36 and 42 nt per fold against the kernels compiled for the CPU.  The energies are integers: equal.
    The defects differ by the compilers' fused multiply-adds: 1e-12, the bound tests/test_edef_lds_gpu.py and
    tests/test_cofold_edef_gpu.py hold between the two."""
    from tests.emu import emu_ragged_aux
    lens = (12, 36, 42)
    seqs, structs = [gold[n][0] for n in lens], [gold[n][1] for n in lens]
    eng.set_targets_ragged(structs)
    ed = eng.ensemble_defect_ragged(seqs, [0, 1, 2])
    E2, E12 = eng.subopt_energy_ragged(seqs, want_both=True)
    jobs = [("ragged", "edef_lds" if n <= 40 else "edef_general", seqs, [k], structs, 42, 64) for k, n in enumerate(lens)]
    jobs += [("ragged", "subopt_lds", seqs, [k], None, 42, 64) for k in range(3)]
    out = emu_ragged_aux.run_jobs(jobs)
    for k, n in enumerate(lens):
        d = abs(float(out[k]["edef"][k]) - float(ed[k]))
        print("%d nt: edef %.15f, |GPU - emulation| %.3e" % (n, ed[k], d))
        assert out[k]["status"][k] == 0 and d < 1e-12, n
        assert int(out[3 + k]["E2"][k]) == int(E2[k]) and out[3 + k]["E12"][k].tolist() == E12[k].tolist(), n


# ---- the native loop

@pytest.fixture(scope="module")
def start(eng, gold):
    """The five problems; every chain starts from its puzzle's golden solution: the state from ONE ragged score, plus the start's
    second-best energy and ensemble defect"""
    from desirna_amd import design, engine as E
    hk = E.HostKernels()
    probs = [design.DesignProblem(gold[n][1]) for n in MC_LENS]
    seqs = [gold[n][0] for n in MC_LENS for _ in range(MC_R)]
    tof = [k for k in range(len(MC_LENS)) for _ in range(MC_R)]
    eng.set_targets_ragged([p.sec_struct for p in probs])
    out = eng.score_ragged(seqs, tof)
    edef = eng.ensemble_defect_ragged(seqs, tof)
    sub = eng.subopt_energy_ragged(seqs) / 100.0
    states = []
    for k, p in enumerate(probs):
        rows = slice(k * MC_R, (k + 1) * MC_R)
        ss = np.frombuffer("".join(out["mfe_ss"][rows]).encode(), np.uint8).reshape(MC_R, p.n).copy()
        mcc, _, _ = hk.simscore(p.sec_struct, ss)
        assert (mcc == 1).all(), "the golden solution of %d nt does not fold to its target" % p.n
        states.append(dict(seqs=np.frombuffer("".join(seqs[rows]).encode(), np.uint8).reshape(MC_R, p.n).copy(), mfe_ss=ss, mcc1=1 - mcc,
                           Epf=out["Epf"][rows].copy(), Ed=out["Ed"][rows] / 100.0, edef=edef[rows].copy(), sub=sub[rows].copy()))
    return SimpleNamespace(probs=probs, states=states, hk=hk)


def _start_scores(st, sf, nd):
    """the -sf sum of a (solved) start state, minus the negative-design term (its value only has to be the same on both sides)"""
    term = {"Ed-Epf": st["Ed"] - st["Epf"], "Edef": st["edef"]}
    tot = sum(term[name] * w for name, w in sf)
    return tot - (st["sub"] - st["Epf"]) if nd else tot


@pytest.mark.parametrize("sf,nd", [([("Ed-Epf", 1.0)], True), ([("Ed-Epf", 0.5), ("Edef", 5.0)], False),
                                   ([("Ed-Epf", 0.5), ("Edef", 5.0)], True)], ids=["nd", "edef", "both"])
def test_mc_run_ragged_nd_equals_mc_run_nd_per_puzzle(eng, start, sf, nd):
    from desirna_amd import engine as E
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL
    hk, probs, R = start.hk, start.probs, MC_R
    nv = 4 + nd
    keys = ("seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed")
    c0 = eng.get_option("edef_lds_calls")
    per = []
    for p, st0 in zip(probs, start.states):
        eng.set_targets([p.sec_struct])
        st = {k: st0[k].copy() for k in ("seqs", "mfe_ss", "mcc1", "Epf", "Ed")}
        st["score"] = _start_scores(st0, sf, nd)
        sub = st0["sub"].copy() if nd else None
        best = dict(seq=st["seqs"][0].copy(), ss=st["mfe_ss"][0].copy(), vals=np.array([2.0, 0.0, 0.0, 0.0, 0.0][:nv]))
        counters, rng = np.zeros(3, np.int64), hk.rng_seed(np.arange(R))
        eng.mc_run(p, N_ITER, np.arange(R, dtype=np.int32), R, 0.7, 0.0, True, np.linspace(10, 150, R), sf, flags, rng, st, counters, best,
                   subopt_e=sub)
        per.append((st, best, counters, rng, sub))
    c1 = eng.get_option("edef_lds_calls")
    P = len(probs)
    state = {k: np.concatenate([st0[k].ravel() for st0 in start.states]) for k in ("seqs", "mfe_ss", "mcc1", "Epf", "Ed")}
    state["score"] = np.concatenate([_start_scores(st0, sf, nd) for st0 in start.states])
    sub = np.concatenate([st0["sub"] for st0 in start.states]) if nd else None
    best = dict(seq=np.concatenate([st0["seqs"][0] for st0 in start.states]), ss=np.concatenate([st0["mfe_ss"][0] for st0 in start.states]),
                vals=np.tile(np.array([2.0, 0.0, 0.0, 0.0, 0.0][:nv]), (P, 1)))
    counters = np.zeros((P, 3), np.int64)
    rng = np.concatenate([hk.rng_seed(np.arange(R)) for _ in probs])
    eng.mc_run_ragged_nd(probs, N_ITER, np.tile(np.arange(R, dtype=np.int32), P), [R] * P, 0.7, 0.0, True,
                         np.tile(np.linspace(10, 150, R), P), sf, flags, rng, state, counters, best, subopt_e=sub)
    if any(name == "Edef" for name, _ in sf):
        # alone, the two puzzles of at most 40 nt make one fused launch per iteration each; in the set they share one
        assert c1 - c0 == 2 * N_ITER and eng.get_option("edef_lds_calls") - c1 == N_ITER
    assert (counters[:, 0] + counters[:, 2]).tolist() == [N_ITER * R] * P and counters[:, 0].all()       # every puzzle moved
    oc = ol = ob = 0
    for k, (p, st0, (st, bst, cnt, rg, sb)) in enumerate(zip(probs, start.states, per)):
        for key in ("seqs", "mfe_ss"):
            assert state[key][ol:ol + R * p.n].tobytes() == st[key].tobytes(), (p.n, key)
        for key in ("score", "mcc1", "Epf", "Ed"):
            assert state[key][oc:oc + R].tobytes() == st[key].tobytes(), (p.n, key)
        assert rng[oc:oc + R].tobytes() == rg.tobytes(), p.n
        assert counters[k].tobytes() == cnt.tobytes(), p.n
        assert best["seq"][ob:ob + p.n].tobytes() == bst["seq"].tobytes() and best["ss"][ob:ob + p.n].tobytes() == bst["ss"].tobytes()
        assert best["vals"][k].tobytes() == bst["vals"].tobytes(), p.n
        if nd:
            assert sub[oc:oc + R].tobytes() == sb.tobytes(), p.n
            # an accepted solved proposal went through the negative-design step inside the loop
            moved = [r for r in range(R) if st["mcc1"][r] == 0 and sb[r] != 0 and st["seqs"][r].tobytes() != st0["seqs"][r].tobytes()]
            assert moved, "%d nt: no chain ends solved, with a second-best energy, away from its start: other stream seeds" % p.n
        oc, ol, ob = oc + R, ol + R * p.n, ob + p.n


def test_batch_driver_with_nd_and_edef_equals_fast_driver_per_puzzle(eng, monkeypatch):
    from desirna_amd import design
    from desirna_amd import energy_scores as es
    # more than one -sf term: the reference keeps the first only (parse_scoring_functions); all of them here
    monkeypatch.setattr(es, "parse_scoring_functions", lambda s, first_term_only=True, _p=es.parse_scoring_functions: _p(s, False))
    targets = {r["name"]: r["structure"] for r in csv.DictReader(open(os.path.join(GOLDEN, "eterna_v1_targets.csv")))}
    inputs = [_input(name, targets[name]) for name in ("eteV1_01.txt", "eteV1_03.txt", "eteV1_16.txt")]
    assert [len(i.sec_struct) for i in inputs] == [16, 36, 105]
    kw = dict(negative_design="on", scoring_f="Ed-Epf:0.5,Edef:5.0", replicas=4, exchange=10, steps=3, seed=5, engine=eng)
    c0 = eng.get_option("edef_lds_calls")
    got = design.run_puzzle_batch(inputs, **kw)
    c1 = eng.get_option("edef_lds_calls")
    # one fused launch for the initial sequences and one per iteration, shared by the 16- and the 36-nt puzzle: not one per puzzle
    assert c1 - c0 == 1 + kw["steps"] * kw["exchange"]
    for inp, a in zip(inputs, got):
        b = design.run_design_fast(inp, **kw)
        assert a["used_native_loop"] is True and b["used_native_loop"] is True
        assert len(a["simulation_data"]) == len(b["simulation_data"])
        for k in KEYS + ("subopt_e", "esubopt_minus_Epf", "mcc", "Epf", "edesired"):
            assert [r[k] for r in a["simulation_data"]] == [r[k] for r in b["simulation_data"]], (inp.name, k)
        for k in COUNTERS:
            assert a["stats"][k] == b["stats"][k], (inp.name, k)
        assert vars(a["best"]) == vars(b["best"]) and a["steps"] == b["steps"] and a["solved"] == b["solved"]
        assert hasattr(a["best"], "subopt_e")
    assert eng.get_option("edef_lds_calls") - c1 == 2 * (1 + kw["steps"] * kw["exchange"])


def _nd_call(engine, probs, Rs, sf=(("Ed-Epf", 1.0), ("Edef", 1.0)), n_iter=1):
    from desirna_amd import engine as E
    C, letters = sum(Rs), sum(R * p.n for p, R in zip(probs, Rs))
    state = dict(seqs=np.full(letters, ord("A"), np.uint8), mfe_ss=np.full(letters, ord("."), np.uint8),
                 **{k: np.zeros(C) for k in ("score", "mcc1", "Epf", "Ed")})
    chars = sum(p.n for p in probs)
    best = dict(seq=np.full(chars, ord("A"), np.uint8), ss=np.full(chars, ord("."), np.uint8), vals=np.zeros((len(probs), 5)))
    engine.mc_run_ragged_nd(probs, n_iter, np.zeros(C, np.int32), Rs, 0.7, 0.0, True, np.full(C, 10.0), list(sf),
                            E.NEED_PF | E.NEED_MFE | E.NEED_EVAL, E.HostKernels().rng_seed(np.arange(C)), state,
                            np.zeros((len(probs), 3), np.int64), best, subopt_e=np.zeros(C))


def test_argument_errors_of_the_three_symbols(eng, gold):
    from desirna_amd import design, engine as E
    p12, p36 = design.DesignProblem(gold[12][1]), design.DesignProblem(gold[36][1])
    s12, s36 = gold[12][0], gold[36][0]
    eng.set_targets_ragged([gold[12][1], gold[36][1]])
    long = "A" * (eng.max_L + 1)
    cases = [
        (lambda: eng.ensemble_defect_ragged([s12, long], [0, 1]), "drna_ensemble_defect_ragged", "max_L"),
        (lambda: eng.subopt_energy_ragged([s12, long]), "drna_subopt_energy_ragged", "max_L"),
        (lambda: _nd_call(eng, [p12, design.DesignProblem("." * (eng.max_L + 1))], [2, 2]), "drna_mc_run_ragged_nd", "max_L"),
        (lambda: eng.ensemble_defect_ragged([s12, s36], [1, 1]), "drna_ensemble_defect_ragged", "with the sequence's length"),
        (lambda: eng.ensemble_defect_ragged([s12, s36], [0, 2]), "drna_ensemble_defect_ragged", "target_of"),
        (lambda: eng.ensemble_defect_ragged([s12] * (eng.max_R + 1), [0] * (eng.max_R + 1)), "drna_ensemble_defect_ragged", "max_R"),
        (lambda: eng.subopt_energy_ragged([s12] * (eng.max_R + 1)), "drna_subopt_energy_ragged", "max_R"),
        (lambda: _nd_call(eng, [p12, p36], [eng.max_R, 1]), "drna_mc_run_ragged_nd", "max_R = %d" % eng.max_R),
        (lambda: _nd_call(eng, [p12, design.DesignProblem("((((....&....))))")], [2, 2]), "drna_mc_run_ragged_nd", "'&'"),
        (lambda: _nd_call(eng, [design.DesignProblem("((((..[[[..))))...]]]"), p12], [2, 2]), "drna_mc_run_ragged_nd", "'['"),
    ]
    for call, who, cause in cases:
        with pytest.raises(E.EngineError) as err:
            call()
        assert err.value.code == -1 and who in str(err.value) and cause in str(err.value), (who, cause, str(err.value))
    # the old symbol still refuses the term the new one accepts
    from tests.test_puzzle_set_gpu import _ragged_call
    with pytest.raises(E.EngineError, match="Edef"):
        _ragged_call(eng, [p12, p36], [2, 2], (("Edef", 1.0),))
    _nd_call(eng, [p12, p36], [2, 2])


def test_ragged_scoring_is_the_same_around_a_set_call_with_aux_folds(eng, start):
    """score_ragged, a drna_mc_run_ragged_nd call with both switches (it replaces the ragged targets by its own, two of the five,
    and uses the ensemble-defect and second-best descriptor blocks), the targets installed again, score_ragged; the auxiliary entry
    points likewise"""
    probs = start.probs
    structs = [p.sec_struct for p in probs]
    seqs = [bytes(r).decode() for st in start.states for r in st["seqs"]]
    tof = [k for k, st in enumerate(start.states) for _ in st["seqs"]]
    eng.set_targets_ragged(structs)
    before = eng.score_ragged(seqs, tof)
    ed0, sub0 = eng.ensemble_defect_ragged(seqs, tof), eng.subopt_energy_ragged(seqs)
    _nd_call(eng, [probs[1], probs[3]], [3, 2], n_iter=3)
    eng.set_targets_ragged(structs)
    after = eng.score_ragged(seqs, tof)
    for k in ("Epf", "Emfe", "Ed"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert before["mfe_ss"] == after["mfe_ss"]
    assert ed0.tobytes() == eng.ensemble_defect_ragged(seqs, tof).tobytes() and sub0.tobytes() == eng.subopt_energy_ragged(seqs).tobytes()
