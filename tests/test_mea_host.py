"""--structures on the host side, with an oracle-backed stand-in engine (no GPU): the rows of design.structure_report for one
strand and two, the CSV text and its rounding, the flag's parsing (needs -o, a weight > 0, works with --set, takes two strands),
that nothing happens without it and that --ensemble is as it was."""
import csv
import math
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design, outputs
from tests import mea_ref as mr
from tests.test_puzzle_set_host import HAIRPIN14, RaggedOracleEngine

KT = 1.98717e-3 * 310.15


class MeaOracleEngine(RaggedOracleEngine):
    """the stand-in engine plus counted score_batch / mea_structures: the oracle's fold and pair probabilities, the numpy
    recurrence of tests/mea_ref.py on them"""
    max_R = 4

    def __init__(self, oracle):
        super().__init__(oracle)
        self.mea_calls, self.score_sizes = [], []

    def score_batch(self, seqs, flags=0):
        self.score_sizes.append(len(seqs))
        folds = [self.o.mfe(s) for s in seqs]
        return {"Epf": np.array([self.o.pf(s) for s in seqs]), "Emfe": np.array([e for _, e in folds], dtype=np.int32),
                "mfe_ss": [ss for ss, _ in folds], "Ed": None}

    def mea_structures(self, seqs, gamma=1.0, want_bpp=False):
        self.mea_calls.append((list(seqs), gamma))
        out = {"mea": [], "mea_value": [], "centroid": [], "centroid_distance": [], "E": []}
        for s in seqs:
            _, P = self.o.ensemble_defect(s, "." * len(s), want_bpp=True)
            db, val = mr.mea(P, gamma)
            cen, dist = mr.centroid(P)
            out["mea"].append(db); out["mea_value"].append(val); out["centroid"].append(cen); out["centroid_distance"].append(dist)
            out["E"].append([self.o.eval_structure(s, db), self.o.eval_structure(s, cen)])
        return {k: (v if k in ("mea", "centroid") else np.array(v)) for k, v in out.items()}


def _input_file(tmp_path, name, ss):
    f = tmp_path / (name + ".txt")
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss))
    return str(f)


def _run_cli(monkeypatch, tmp_path, oracle, extra, source=None):
    eng = MeaOracleEngine(oracle)
    real = design.run_design_fast
    monkeypatch.setattr(design, "run_design_fast", lambda inp, **kw: real(inp, engine=eng, **dict(kw, native_loop=False)))
    real_batch = design.run_puzzle_batch
    monkeypatch.setattr(design, "run_puzzle_batch", lambda inputs, **kw: real_batch(inputs, engine=eng, **dict(kw, native_loop=False)))
    out = tmp_path / "out"
    source = source or ["-f", _input_file(tmp_path, "hp", HAIRPIN14)]
    design.main(source + ["-R", "4", "-e", "5", "-s", "2", "-seed", "3", "-r", "6", "-o", str(out)] + extra)
    return eng, out


def test_report_rows(monkeypatch, tmp_path, oracle):
    eng, out = _run_cli(monkeypatch, tmp_path, oracle, ["--structures", "2.0"])
    (res_file,) = [p for p in out.iterdir() if p.name.endswith("_results.csv")]
    (st_file,) = [p for p in out.iterdir() if p.name.endswith("_structures.csv")]
    assert st_file.name == res_file.name.replace("_results.csv", "_structures.csv")
    reported = [r["sequence"] for r in csv.DictReader(open(res_file))]
    assert eng.mea_calls == [(reported, 2.0)]                    # one call for the puzzle, the reported sequences in their order
    assert sum(eng.score_sizes) == len(reported) and max(eng.score_sizes) <= eng.max_R
    rows = list(csv.DictReader(open(st_file)))
    assert tuple(rows[0].keys()) == outputs.STRUCTURE_COLUMNS
    assert [r["sequence"] for r in rows] == [s for s in reported for _ in range(3)]
    for seq in reported:
        mfe, cen, mea = [r for r in rows if r["sequence"] == seq]
        assert [mfe["kind"], cen["kind"], mea["kind"]] == ["mfe", "centroid", "mea"]
        _, P = oracle.ensemble_defect(seq, "." * len(seq), want_bpp=True)
        assert (mfe["structure"], round(oracle.mfe(seq)[1] / 100.0, 3)) == (oracle.mfe(seq)[0], float(mfe["energy"]))
        assert cen["structure"] == mr.centroid(P)[0] and abs(float(cen["value"]) - mr.centroid(P)[1]) < 1e-3
        assert mea["structure"] == mr.mea(P, 2.0)[0] and abs(float(mea["value"]) - mr.mea(P, 2.0)[1]) < 1e-3
        assert mfe["value"] == ""
        for r in (mfe, cen, mea):
            e = oracle.eval_structure(seq, r["structure"]) / 100.0
            assert abs(float(r["energy"]) - e) < 1e-9 and abs(float(r["Epf"]) - oracle.pf(seq)) < 1e-3
            assert abs(float(r["p_structure"]) - math.exp(-(e - oracle.pf(seq)) / KT)) < 1e-3
            assert 0.0 <= float(r["mcc"]) <= 2.0
            assert (float(r["mcc"]) == 0.0) == (r["structure"] == HAIRPIN14)


def test_nothing_without_the_flag_and_ensemble_as_before(monkeypatch, tmp_path, oracle):
    eng, out = _run_cli(monkeypatch, tmp_path, oracle, [])
    assert eng.mea_calls == [] and eng.score_sizes == []
    assert not [p for p in out.iterdir() if "structures" in p.name]
    assert [p for p in out.iterdir() if p.name.endswith("_results.csv")]
    # --ensemble still refuses two strands and still needs -o; --structures beside it changes neither
    two = _input_file(tmp_path, "two", "((((....&....))))")
    monkeypatch.setattr(design, "run_design_fast", lambda *a, **k: pytest.fail("a run was started"))
    monkeypatch.setattr(design, "run_design", lambda *a, **k: pytest.fail("a run was started"))
    for argv in (["-f", two, "--ensemble", "16", "-o", str(tmp_path / "o")],
                 ["-f", two, "--ensemble", "16", "--structures", "1", "-o", str(tmp_path / "o")],
                 ["-f", two, "--ensemble", "16"]):
        with pytest.raises(SystemExit) as ex:
            design.main(argv)
        assert ex.value.code == 2


def test_flag_parsing(monkeypatch, tmp_path, capsys):
    one = _input_file(tmp_path, "hp", HAIRPIN14)
    two = _input_file(tmp_path, "two", "((((....&....))))")

    class Started(Exception):
        pass

    def started(*a, **k):
        raise Started()

    monkeypatch.setattr(design, "run_design_fast", started)
    monkeypatch.setattr(design, "run_design", started)
    monkeypatch.setattr(design, "run_puzzle_set", started)
    o = str(tmp_path / "o")
    for argv, word in ((["--structures", "1.0"], "give -o"), (["--structures", "0", "-o", o], "GAMMA > 0"),
                       (["--structures", "-2", "-o", o], "GAMMA > 0"), (["--structures", "inf", "-o", o], "GAMMA > 0"),
                       (["--structures", "nan", "-o", o], "GAMMA > 0"), (["--structures", "x", "-o", o], "invalid float")):
        with pytest.raises(SystemExit) as ex:
            design.main(["-f", one] + argv)
        assert ex.value.code == 2 and word in capsys.readouterr().err
    # accepted: one strand, two strands, a set with a two-strand member -- the run starts
    for argv in (["-f", one], ["-f", two], ["--set", one, two]):
        with pytest.raises(Started):
            design.main(argv + ["--structures", "0.5", "-o", o])


def test_set_writes_a_file_per_puzzle(monkeypatch, tmp_path, oracle):
    files = [_input_file(tmp_path, "hp", HAIRPIN14), _input_file(tmp_path, "hq", "(((....)))....")]
    eng, out = _run_cli(monkeypatch, tmp_path, oracle, ["--structures", "1"], source=["--set"] + files)
    st = sorted(p.name for p in out.iterdir() if p.name.endswith("_structures.csv"))
    assert len(st) == 2 and st[0].startswith("hp_") and st[1].startswith("hq_")
    for p in out.iterdir():
        if p.name.endswith("_structures.csv"):
            rows = list(csv.DictReader(open(p)))
            assert rows and len(rows) % 3 == 0 and {r["kind"] for r in rows} == {"mfe", "centroid", "mea"}


class TwoStrandStub:
    """canned answers for one pair: what Engine.cofold_batch / cofold_mea_structures return"""
    max_R = 8

    def cofold_batch(self, seqs, flags=0):
        assert seqs == ["GGGGAA&AACCCC"]
        return {"mfe_ss": ["((((..&..))))"], "Emfe": np.array([-510], dtype=np.int32), "FAB": np.array([-5.4]), "Ed": None}

    def cofold_mea_structures(self, seqs, gamma=1.0, want_bpp=False):
        assert seqs == ["GGGGAA&AACCCC"] and gamma == 0.5
        return {"mea": ["((((..&..))))"], "mea_value": np.array([7.123456]), "centroid": [".(((..&..)))."],
                "centroid_distance": np.array([0.98765]), "E": np.array([[-510, -320]], dtype=np.int32)}


def test_two_strand_rows_and_csv_rounding():
    inp = SimpleNamespace(name="two", sec_struct="((((..&..))))")
    rows = design.structure_report(TwoStrandStub(), {"reported": ["GGGGAA&AACCCC"]}, inp, gamma=0.5)
    assert [r["kind"] for r in rows] == ["mfe", "centroid", "mea"]
    assert [r["structure"] for r in rows] == ["((((..&..))))", ".(((..&..))).", "((((..&..))))"]
    assert [r["energy"] for r in rows] == [-5.1, -3.2, -5.1] and all(r["Epf"] == -5.4 for r in rows)
    assert [r["value"] for r in rows] == ["", 0.98765, 7.123456]
    assert rows[0]["mcc"] == 0.0 and rows[2]["mcc"] == 0.0 and 0.0 < rows[1]["mcc"] <= 2.0       # '&' -> 'Ee' on both sides
    assert abs(rows[0]["p_structure"] - math.exp(-0.3 / KT)) < 1e-12
    text = outputs.structures_csv_text(rows)
    lines = text.splitlines()
    assert lines[0] == ",".join(outputs.STRUCTURE_COLUMNS) and len(lines) == 4
    assert lines[1] == "GGGGAA&AACCCC,-5.4,mfe,((((..&..)))),-5.1,%s,,0.0" % round(math.exp(-0.3 / KT), 3)
    assert lines[2].split(",")[6] == "0.988" and lines[3].split(",")[6] == "7.123"
