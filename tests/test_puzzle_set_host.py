"""Puzzle sets in lock-step, host side: design.run_puzzle_batch on an oracle-backed stand-in engine (per-iteration loop, one ragged
scoring call per iteration) against design.run_design_fast of every puzzle alone; the routing of run_puzzle_set(batched=True)
and of the command line's --set."""
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design
from tests.test_design_driver import ETE1, OracleEngine

HAIRPIN14 = "((((......))))"
KEYS = ("sequence", "mfe_ss", "temp_shelf", "sim_step", "scoring_function")
COUNTERS = ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored")
KW = dict(replicas=4, exchange=10, seed=5)


class RaggedOracleEngine(OracleEngine):
    """OracleEngine plus a counted score_ragged_arrays; rectangular score calls are counted too (the batch driver makes none)"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.ragged_calls, self.ragged_sizes, self.rect_calls = 0, [], 0

    def set_targets_ragged(self, structures):
        self.ragged_targets = list(structures)

    def score_batch_arrays(self, seqs_u8, flags=0):
        self.rect_calls += 1
        return super().score_batch_arrays(seqs_u8, flags)

    def score_ragged_arrays(self, flat_u8, lens, target_of=None, flags=0):
        self.ragged_calls += 1
        self.ragged_sizes.append(len(lens))
        flat = bytes(np.asarray(flat_u8, dtype=np.uint8)).decode()
        offs = np.concatenate(([0], np.cumsum(lens)))
        R = len(lens)
        Epf, Emfe, Ed, ss = np.zeros(R), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32), [None] * R
        for t in sorted(set(int(x) for x in target_of)):           # one oracle batch per structure
            rows = [r for r in range(R) if target_of[r] == t]
            e, m, s, d = self.o.score_batch([flat[offs[r]:offs[r + 1]] for r in rows], [self.ragged_targets[t]], threads=4)
            for k, r in enumerate(rows):
                Epf[r], Emfe[r], ss[r], Ed[r] = e[k], m[k], s[k], d[k][0]
        return Epf, Emfe, np.frombuffer("".join(ss).encode(), dtype=np.uint8).copy(), Ed


def _input(name, ss):
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr="N" * len(ss), seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


@pytest.fixture(scope="module")
def puzzles(example_inputs):
    return [_input("hairpin14", HAIRPIN14), _input("eteV1_01", ETE1),
            _input("standard36", example_inputs["Standard_design_input"]["sec_struct"][0])]


def _same_run(a, b):
    """the batch's result for one puzzle against that puzzle's run alone"""
    assert len(a["simulation_data"]) == len(b["simulation_data"])
    for k in KEYS:
        assert [r[k] for r in a["simulation_data"]] == [r[k] for r in b["simulation_data"]], k
    for k in COUNTERS:
        assert a["stats"][k] == b["stats"][k], k
    assert vars(a["best"]) == vars(b["best"])
    assert a["steps"] == b["steps"] and a["solved"] == b["solved"] and a["temps"] == b["temps"]
    assert a["used_native_loop"] is False and b["used_native_loop"] is False


def test_batch_equals_every_puzzle_alone(oracle, puzzles):
    steps = 3
    eng = RaggedOracleEngine(oracle)
    got = design.run_puzzle_batch(puzzles, steps=steps, native_loop=False, engine=eng, **KW)
    assert len(got) == len(puzzles)
    for inp, a in zip(puzzles, got):
        _same_run(a, design.run_design_fast(inp, steps=steps, native_loop=False, engine=OracleEngine(oracle), **KW))
        assert a["steps"] == steps
    # one ragged call for the initial sequences, then exactly one per iteration, always with every chain; nothing rectangular
    assert eng.ragged_calls == 1 + steps * KW["exchange"] and eng.rect_calls == 0
    assert set(eng.ragged_sizes) == {len(puzzles) * KW["replicas"]}


# (seed, step count and exchange interval chosen with the oracle: both hairpins are solved by their initial sequence, the 36-nt
# target after a few iterations; under the -sws rule, tested every 10th step, the hairpins hold 8 distinct solved sequences at
# step 10 and the 36-nt target does not)
@pytest.mark.parametrize("kw", [dict(replicas=4, exchange=10, seed=1, steps=1),
                                dict(replicas=4, exchange=2, seed=5, steps=20, num_results=8)], ids=["first_solved", "sws"])
def test_a_stopped_puzzle_leaves_the_batch(oracle, puzzles, kw):
    steps = kw["steps"]
    kw = dict(kw, stop_when_solved=True, native_loop=False)
    eng = RaggedOracleEngine(oracle)
    got = design.run_puzzle_batch(puzzles, engine=eng, **kw)
    for inp, a in zip(puzzles, got):
        _same_run(a, design.run_design_fast(inp, engine=OracleEngine(oracle), **kw))
    n_steps = [a["steps"] for a in got]
    assert min(n_steps) < steps, "no puzzle stopped early: the case shows nothing"
    assert max(n_steps) == steps, "no puzzle ran to its step count"
    R, ex = kw["replicas"], kw["exchange"]
    # step s holds the chains of the puzzles that reached it
    want = [len(puzzles) * R] + [R * sum(n >= s for n in n_steps) for s in range(1, steps + 1) for _ in range(ex)]
    assert eng.ragged_sizes == want and eng.rect_calls == 0
    assert eng.ragged_sizes[-1] < eng.ragged_sizes[0]


def test_batch_refuses_what_it_cannot_run(puzzles):
    for bad in (_input("two", "((((....&....))))"), _input("pk", "((((..[[[..))))...]]]"),
                SimpleNamespace(**dict(vars(puzzles[0]), alt_sec_structs=[".(((......)))."]))):
        assert not design.batch_eligible(bad)
        with pytest.raises(ValueError):
            design.run_puzzle_batch([puzzles[0], bad], steps=1, engine=object(), **KW)
    assert design.batch_eligible(puzzles[0])
    assert not design.batch_eligible(puzzles[0], negative_design="on") and not design.batch_eligible(puzzles[0], oligo="on")
    assert not design.batch_eligible(puzzles[0], scoring_f="Edef:1.0") and not design.batch_eligible(puzzles[0], acgu={"A": 25})


def _fake_result(tag):
    best = SimpleNamespace(sequence=tag, mfe_ss="." * 3, Epf=0.0, edesired=0.0, mcc=1.0, scoring_function=0.0)
    return {"best": best, "solved": False, "steps": 0, "stats": {"scored": 0, "elapsed_s": 0.0}}


def test_puzzle_set_routes_eligible_inputs_to_the_batch(monkeypatch, puzzles):
    two = _input("two", "((((....&....))))")
    alt = SimpleNamespace(**dict(vars(_input("alt", HAIRPIN14)), alt_sec_structs=[".(((......)))."], alt_sec_struct=".(((......)))."))
    inputs = [puzzles[0], two, puzzles[1], alt, puzzles[2]]
    seen = []

    def batch(inps, **kw):
        seen.append(("batch", [i.name for i in inps], kw))
        return [_fake_result("batch:" + i.name) for i in inps]

    def driver(inp, **kw):
        seen.append(("driver", inp.name, kw))
        return _fake_result("driver:" + inp.name)

    monkeypatch.setattr(design, "run_puzzle_batch", batch)
    out = design.run_puzzle_set(inputs, driver=driver, batched=True, replicas=4, steps=2)
    assert [s[:2] for s in seen] == [("batch", ["hairpin14", "eteV1_01", "standard36"]), ("driver", "two"), ("driver", "alt")]
    assert all(s[2] == dict(replicas=4, steps=2) for s in seen)
    assert [out[k]["name"] for k in range(5)] == [i.name for i in inputs]
    assert [out[k]["sequence"] for k in range(5)] == ["batch:hairpin14", "driver:two", "batch:eteV1_01", "driver:alt", "batch:standard36"]
    # the default stays per puzzle; -nd on sends everything to the driver
    seen.clear()
    design.run_puzzle_set(inputs[:3], driver=driver, replicas=4)
    design.run_puzzle_set(inputs[:3], driver=driver, batched=True, negative_design="on")
    assert [s[0] for s in seen] == ["driver"] * 6


def test_cli_set_reaches_the_batched_puzzle_set(monkeypatch, tmp_path, capsys):
    files = []
    for name, ss in (("a", HAIRPIN14), ("b", ETE1)):
        f = tmp_path / (name + ".txt")
        f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss))
        files.append(str(f))
    for argv in ([], ["-R", "4"], ["-f", files[0], "--set", files[1]]):
        with pytest.raises(SystemExit):
            design.main(argv)
    capsys.readouterr()
    seen = []

    def fake_set(inputs, **kw):
        seen.append(([i.name for i in inputs], kw))
        for k, inp in enumerate(inputs):
            kw["on_result"](k, inp, _fake_result("X" * len(inp.sec_struct)))
        return {}

    monkeypatch.setattr(design, "run_puzzle_set", fake_set)
    design.main(["--set"] + files + ["-R", "4", "-s", "2"])
    (names, kw), = seen
    assert names == ["a", "b"] and kw["batched"] is True and kw["replicas"] == 4 and kw["steps"] == 2
    assert kw["negative_design"] == "off" and kw["oligo"] == "off" and "acgu" not in kw
    assert capsys.readouterr().out.count("Design not solved.") == 2          # every puzzle is reported as -f reports its one


def test_cli_set_runs_the_batch_and_writes_each_puzzles_files(monkeypatch, tmp_path, oracle):
    """--set end to end on the stand-in engine: the eligible puzzles share one batch, -o gets every puzzle's result files"""
    files = []
    for name, ss in (("a", HAIRPIN14), ("b", ETE1)):
        f = tmp_path / (name + ".txt")
        f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss))
        files.append(str(f))
    eng = RaggedOracleEngine(oracle)
    real = design.run_puzzle_batch
    monkeypatch.setattr(design, "run_puzzle_batch", lambda inps, **kw: real(inps, engine=eng, **dict(kw, native_loop=False)))
    out = tmp_path / "out"
    design.main(["--set"] + files + ["-R", "3", "-e", "5", "-s", "2", "-seed", "3", "-o", str(out)])
    assert eng.ragged_calls == 1 + 2 * 5 and eng.rect_calls == 0
    written = sorted(p.name for p in out.iterdir())
    assert any(n.startswith("a") for n in written) and any(n.startswith("b") for n in written)
    assert sum(n.endswith("_results.csv") for n in written) == 2
