"""Puzzle sets in lock-step on the GPU: drna_mc_run_ragged against drna_mc_run of every puzzle alone (bit for bit), the batch
driver on the native loop against run_design_fast per puzzle, the entry point's argument errors, and the ragged plan."""
import csv
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_puzzle_set_host import COUNTERS, KEYS, _input

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 12 nt: the shortest target; 36 nt; 151 nt: alone it takes the fused multi-workgroup launch (>= 125 nt), in the ragged call the
# one-workgroup kernels; 202 nt: the shortest above 200, strips on both sides
MC_PUZZLES = (("eteV1_08.txt", 4), ("eteV1_03.txt", 4), ("eteV1_36.txt", 6), ("eteV1_98.txt", 4))
N_ITER = 12


@pytest.fixture(scope="module")
def targets():
    return {r["name"]: r["structure"] for r in csv.DictReader(open(os.path.join(GOLDEN, "eterna_v1_targets.csv")))}


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine as E
    e = E.Engine(max_R=sum(r for _, r in MC_PUZZLES), max_L=202)
    yield e
    e.close()


@pytest.fixture(scope="module")
def start(eng, targets):
    """The four problems, and per problem its chains' random start sequences with their state from ONE score_ragged call"""
    from desirna_amd import design, engine as E
    hk = E.HostKernels()
    probs = [design.DesignProblem(targets[name]) for name, _ in MC_PUZZLES]
    assert [p.n for p in probs] == [12, 36, 151, 202]
    seqs = [[p.initial_sequence(random.Random(100 * k + c)) for c in range(R)] for k, (p, (_, R)) in enumerate(zip(probs, MC_PUZZLES))]
    eng.set_targets_ragged([p.sec_struct for p in probs])
    out = eng.score_ragged([s for row in seqs for s in row], [k for k, row in enumerate(seqs) for _ in row])
    states, o = [], 0
    for p, row in zip(probs, seqs):
        R = len(row)
        ss = np.frombuffer("".join(out["mfe_ss"][o:o + R]).encode(), np.uint8).reshape(R, p.n).copy()
        mcc, rec, prec = hk.simscore(p.sec_struct, ss)
        states.append(dict(seqs=np.frombuffer("".join(row).encode(), np.uint8).reshape(R, p.n).copy(), mfe_ss=ss, mcc1=1 - mcc,
                           Epf=out["Epf"][o:o + R].copy(), Ed=out["Ed"][o:o + R] / 100.0))
        o += R
    return SimpleNamespace(probs=probs, states=states, hk=hk)


def _start_scores(st, n, sf):
    """the -sf sum of a start state (its value only has to be the same on both sides)"""
    term = {"Ed-Epf": st["Ed"] - st["Epf"], "1-MCC": st["mcc1"] * 10, "sln_Epf": (st["Epf"] + 0.3759 * n + 5.7534) / 10}
    return sum(term[name] * w for name, w in sf)


@pytest.mark.parametrize("sf", [[("Ed-Epf", 1.0)], [("1-MCC", 0.5), ("sln_Epf", 0.5)]], ids=["Ed-Epf", "1-MCC+sln_Epf"])
def test_mc_run_ragged_equals_mc_run_per_puzzle(eng, start, sf):
    from desirna_amd import engine as E
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL
    hk, probs = start.hk, start.probs
    Rs = [R for _, R in MC_PUZZLES]
    per = []
    for p, st0, R in zip(probs, start.states, Rs):
        # the rectangular side starts from its own score_batch of the same sequences
        eng.set_targets([p.sec_struct])
        Epf, _, ss, Ed = eng.score_batch_arrays(st0["seqs"])
        assert Epf.tobytes() == st0["Epf"].tobytes() and ss.tobytes() == st0["mfe_ss"].tobytes()
        assert (Ed[:, 0] / 100.0).tobytes() == st0["Ed"].tobytes()
        st = dict(seqs=st0["seqs"].copy(), mfe_ss=ss, mcc1=st0["mcc1"].copy(), Epf=Epf, Ed=Ed[:, 0] / 100.0)
        st["score"] = _start_scores(st, p.n, sf)
        best = dict(seq=st["seqs"][0].copy(), ss=st["mfe_ss"][0].copy(), vals=np.array([2.0, 0.0, 0.0, 0.0]))
        counters, rng = np.zeros(3, np.int64), hk.rng_seed(np.arange(R))
        eng.mc_run(p, N_ITER, np.arange(R, dtype=np.int32), R, 0.7, 0.0, True, np.linspace(10, 150, R), sf, flags, rng, st, counters, best)
        per.append((st, best, counters, rng))
    state = {k: np.concatenate([st0[k].ravel() for st0 in start.states]) for k in ("seqs", "mfe_ss", "mcc1", "Epf", "Ed")}
    state["score"] = np.concatenate([_start_scores(st0, p.n, sf) for p, st0 in zip(probs, start.states)])
    best = dict(seq=np.concatenate([st0["seqs"][0] for st0 in start.states]), ss=np.concatenate([st0["mfe_ss"][0] for st0 in start.states]),
                vals=np.tile(np.array([2.0, 0.0, 0.0, 0.0]), (len(probs), 1)))
    counters = np.zeros((len(probs), 3), np.int64)
    rng = np.concatenate([hk.rng_seed(np.arange(R)) for R in Rs])
    eng.mc_run_ragged(probs, N_ITER, np.concatenate([np.arange(R, dtype=np.int32) for R in Rs]), Rs, 0.7, 0.0, True,
                      np.concatenate([np.linspace(10, 150, R) for R in Rs]), sf, flags, rng, state, counters, best)
    assert (counters[:, 0] + counters[:, 2]).tolist() == [N_ITER * R for R in Rs] and counters[:, 0].all()      # every puzzle moved
    oc = ol = ob = 0
    for k, (p, R, (st, bst, cnt, rg)) in enumerate(zip(probs, Rs, per)):
        for key in ("seqs", "mfe_ss"):
            assert state[key][ol:ol + R * p.n].tobytes() == st[key].tobytes(), (p.n, key)
        for key in ("score", "mcc1", "Epf", "Ed"):
            assert state[key][oc:oc + R].tobytes() == st[key].tobytes(), (p.n, key)
        assert rng[oc:oc + R].tobytes() == rg.tobytes(), p.n
        assert counters[k].tobytes() == cnt.tobytes(), p.n
        assert best["seq"][ob:ob + p.n].tobytes() == bst["seq"].tobytes() and best["ss"][ob:ob + p.n].tobytes() == bst["ss"].tobytes()
        assert best["vals"][k].tobytes() == bst["vals"].tobytes(), p.n
        oc, ol, ob = oc + R, ol + R * p.n, ob + p.n


@pytest.mark.parametrize("sws", [False, True], ids=["steps", "stop_when_solved"])
def test_batch_driver_equals_fast_driver_per_puzzle(eng, targets, sws):
    from desirna_amd import design
    inputs = [_input(name, targets[name]) for name in ("eteV1_01.txt", "eteV1_03.txt", "eteV1_16.txt")]
    assert [len(i.sec_struct) for i in inputs] == [16, 36, 105]
    kw = dict(replicas=4, exchange=10, steps=3, seed=5, stop_when_solved=sws, engine=eng)
    got = design.run_puzzle_batch(inputs, **kw)
    for inp, a in zip(inputs, got):
        b = design.run_design_fast(inp, **kw)
        assert a["used_native_loop"] is True and b["used_native_loop"] is True
        assert len(a["simulation_data"]) == len(b["simulation_data"])
        for k in KEYS:
            assert [r[k] for r in a["simulation_data"]] == [r[k] for r in b["simulation_data"]], (inp.name, k)
        for k in COUNTERS:
            assert a["stats"][k] == b["stats"][k], (inp.name, k)
        assert vars(a["best"]) == vars(b["best"]) and a["steps"] == b["steps"] and a["solved"] == b["solved"]


def _ragged_call(engine, probs, Rs, sf=(("Ed-Epf", 1.0),)):
    from desirna_amd import engine as E
    C, letters = sum(Rs), sum(R * p.n for p, R in zip(probs, Rs))
    state = dict(seqs=np.full(letters, ord("A"), np.uint8), mfe_ss=np.full(letters, ord("."), np.uint8),
                 **{k: np.zeros(C) for k in ("score", "mcc1", "Epf", "Ed")})
    chars = sum(p.n for p in probs)
    best = dict(seq=np.full(chars, ord("A"), np.uint8), ss=np.full(chars, ord("."), np.uint8), vals=np.zeros((len(probs), 4)))
    engine.mc_run_ragged(probs, 1, np.zeros(C, np.int32), Rs, 0.7, 0.0, True, np.full(C, 10.0), list(sf),
                         E.NEED_PF | E.NEED_MFE | E.NEED_EVAL, E.HostKernels().rng_seed(np.arange(C)), state,
                         np.zeros((len(probs), 3), np.int64), best)


def test_mc_run_ragged_argument_errors(eng, targets):
    from desirna_amd import design, engine as E
    p12, p36 = design.DesignProblem(targets["eteV1_08.txt"]), design.DesignProblem(targets["eteV1_03.txt"])
    cases = [
        (eng, [p12, p36], [2, 2], (("Edef", 1.0),), "Edef"),
        (eng, [p12, design.DesignProblem("((((....&....))))")], [2, 2], (("Ed-Epf", 1.0),), "'&'"),
        (eng, [design.DesignProblem("((((..[[[..))))...]]]"), p12], [2, 2], (("Ed-Epf", 1.0),), "'['"),
        (eng, [p12, p36], [eng.max_R, 1], (("Ed-Epf", 1.0),), "max_R = %d" % eng.max_R),
    ]
    small = E.Engine(max_R=4, max_L=16)
    try:
        cases.append((small, [p36], [4], (("Ed-Epf", 1.0),), "max_R * max_L"))          # 4 chains fit, 144 nucleotides do not
        for engine, probs, Rs, sf, cause in cases:
            with pytest.raises(E.EngineError) as err:
                _ragged_call(engine, probs, Rs, sf)
            assert err.value.code == -1 and cause in str(err.value), (cause, str(err.value))
    finally:
        small.close()


def test_ragged_scoring_is_the_same_around_a_set_call(eng, start):
    """the plan / run split leaves no state behind: score_ragged, a drna_mc_run_ragged call (which replaces the ragged targets by
    its own, here two of the four), the targets installed again, score_ragged"""
    probs = start.probs
    structs = [p.sec_struct for p in probs]
    seqs = [bytes(r).decode() for st in start.states for r in st["seqs"]]
    tof = [k for k, st in enumerate(start.states) for _ in st["seqs"]]
    eng.set_targets_ragged(structs)
    before = eng.score_ragged(seqs, tof)
    _ragged_call(eng, [probs[1], probs[3]], [3, 2])
    eng.set_targets_ragged(structs)
    after = eng.score_ragged(seqs, tof)
    for k in ("Epf", "Emfe", "Ed"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert before["mfe_ss"] == after["mfe_ss"]
