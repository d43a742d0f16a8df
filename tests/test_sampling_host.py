"""--ensemble on the host side, with an oracle-backed stand-in engine (no GPU): the report's rows and sums, that nothing happens
without the flag, and that two strands are refused when the arguments are parsed."""
import csv
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design, outputs
from tests import sampling_ref as sr
from tests.test_puzzle_set_host import HAIRPIN14, RaggedOracleEngine

S = 64


class SamplingOracleEngine(RaggedOracleEngine):
    """the stand-in engine plus a counted sample_structures: draws with numpy from the exact distribution of each (14-nt) sequence"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.sample_calls = []

    def sample_structures(self, seqs, S, seed=0):
        self.sample_calls.append((list(seqs), S, seed))
        out, E = [], np.zeros((len(seqs), S), dtype=np.int32)
        for r, seq in enumerate(seqs):
            dist = sr.exact_distribution(self.o, seq)
            keys = sorted(dist)
            p = np.array([dist[k] for k in keys])
            pick = np.random.default_rng(seed + r).choice(len(keys), S, p=p / p.sum())
            out.append([keys[k] for k in pick])
            E[r] = [self.o.eval_structure(seq, s) for s in out[-1]]
        return out, E, np.array([self.o.pf(s) for s in seqs])


def _input_file(tmp_path, name, ss):
    f = tmp_path / (name + ".txt")
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss))
    return str(f)


def _run_cli(monkeypatch, tmp_path, oracle, extra):
    eng = SamplingOracleEngine(oracle)
    real = design.run_design_fast
    monkeypatch.setattr(design, "run_design_fast", lambda inp, **kw: real(inp, engine=eng, **dict(kw, native_loop=False)))
    out = tmp_path / "out"
    design.main(["-f", _input_file(tmp_path, "hp", HAIRPIN14), "-R", "4", "-e", "5", "-s", "2", "-seed", "3", "-r", "6", "-o", str(out)] + extra)
    return eng, out


def test_report_rows_and_sums(monkeypatch, tmp_path, oracle):
    eng, out = _run_cli(monkeypatch, tmp_path, oracle, ["--ensemble", str(S), "--ensemble-top", "3", "--ensemble-seed", "11"])
    (res_file,) = [p for p in out.iterdir() if p.name.endswith("_results.csv")]
    (ens_file,) = [p for p in out.iterdir() if p.name.endswith("_ensemble.csv")]
    assert ens_file.name == res_file.name.replace("_results.csv", "_ensemble.csv")
    reported = [r["sequence"] for r in csv.DictReader(open(res_file))]
    (call,) = eng.sample_calls                                  # one call for the puzzle, the reported sequences in their order
    assert call == (reported, S, 11)
    rows = list(csv.DictReader(open(ens_file)))
    assert tuple(rows[0].keys()) == outputs.ENSEMBLE_COLUMNS
    assert [s for k, s in enumerate(r["sequence"] for r in rows) if k == 0 or s != rows[k - 1]["sequence"]] == reported
    for seq in reported:
        mine = [r for r in rows if r["sequence"] == seq]
        kinds = [r["kind"] for r in mine]
        ntop = kinds.count("top")
        assert 1 <= ntop <= 3 and kinds == ["top"] * ntop + ["target", "other"]
        top, target, other = mine[:ntop], mine[ntop], mine[ntop + 1]
        assert [r["rank"] for r in top] == [str(k + 1) for k in range(ntop)]
        counts = [int(r["count"]) for r in top]
        assert counts == sorted(counts, reverse=True) and len({r["structure"] for r in top}) == ntop
        assert target["structure"] == HAIRPIN14 and int(target["count"]) >= 0 and float(target["mcc"]) == 0.0
        in_top = HAIRPIN14 in [r["structure"] for r in top]
        assert sum(counts) + int(other["count"]) + (0 if in_top else int(target["count"])) == S
        for r in top + [target]:
            assert abs(float(r["frequency"]) - int(r["count"]) / S) < 1e-3
            assert sr.well_formed(seq, r["structure"]) and 0.0 <= float(r["mcc"]) <= 2.0
            assert abs(float(r["energy"]) - oracle.eval_structure(seq, r["structure"]) / 100.0) < 1e-9
            assert abs(float(r["Epf"]) - oracle.pf(seq)) < 1e-3
        # the stand-in's draws, counted again
        drawn = eng.sample_structures([seq], S, 11 + reported.index(seq))[0][0]
        assert all(int(r["count"]) == drawn.count(r["structure"]) for r in top + [target])


def test_nothing_without_the_flag(monkeypatch, tmp_path, oracle):
    eng, out = _run_cli(monkeypatch, tmp_path, oracle, [])
    assert eng.sample_calls == []
    assert not [p for p in out.iterdir() if "ensemble" in p.name]
    assert [p for p in out.iterdir() if p.name.endswith("_results.csv")]


def test_report_without_a_ranking_of_its_own(oracle):
    """design.ensemble_report on a driver's result as it stands: the sequences of outputs.sort_and_filter, one call"""
    eng = SamplingOracleEngine(oracle)
    inp = SimpleNamespace(name="hp", sec_struct=HAIRPIN14, seq_restr="N" * 14, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    res = design.run_design_fast(inp, replicas=4, exchange=5, steps=2, seed=3, engine=eng, native_loop=False)
    rows = design.ensemble_report(eng, res, inp, 32, top=2, seed=0)
    want = [r["sequence"] for r in outputs.sort_and_filter(res["simulation_data"])]
    assert eng.sample_calls == [(want, 32, 0)]
    assert [r["sequence"] for r in rows if r["kind"] == "other"] == want


def test_two_strands_are_refused_at_parsing(monkeypatch, tmp_path, capsys):
    two = _input_file(tmp_path, "two", "((((....&....))))")
    one = _input_file(tmp_path, "hp", HAIRPIN14)
    monkeypatch.setattr(design, "run_design_fast", lambda *a, **k: pytest.fail("a run was started"))
    monkeypatch.setattr(design, "run_design", lambda *a, **k: pytest.fail("a run was started"))
    monkeypatch.setattr(design, "run_puzzle_set", lambda *a, **k: pytest.fail("a run was started"))
    for argv in (["-f", two], ["--set", one, two]):
        with pytest.raises(SystemExit) as ex:
            design.main(argv + ["--ensemble", "16", "-o", str(tmp_path / "o")])
        assert ex.value.code == 2
        assert "two-strand" in capsys.readouterr().err
    for argv in (["--ensemble", "16"], ["--ensemble", "-1", "-o", "x"], ["--ensemble", "4", "--ensemble-top", "0", "-o", "x"]):
        with pytest.raises(SystemExit):
            design.main(["-f", one] + argv)
    capsys.readouterr()
