"""Accessible regions on the host side, with an oracle-backed stand-in engine (no GPU) whose unpaired_free_energy comes from the
enumeration of tests/access_ref.py on a 14-nt hairpin target: the >accessible block of an input, the design term in the scorer
and in both drivers, the columns it adds to records, best and _results.csv, how it routes the drivers, the --accessibility report
and its flags, and that a run without block and flags writes what it wrote before."""
import csv
import math
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design, engine, outputs
from desirna_amd import energy_scores as es
from tests import access_ref as ar
from tests.test_puzzle_set_host import HAIRPIN14, RaggedOracleEngine

REGION14 = "....xxxxxx...."                     # the hairpin's loop
KT = 0.001987204259 * (273.15 + 37)             # the kT of energy_scores.kTlog_*


class AccessOracleEngine(RaggedOracleEngine):
    """the stand-in engine plus a counted unpaired_free_energy (enumeration) and score_batch (the oracle's fold)"""
    max_R = 4

    def __init__(self, oracle):
        super().__init__(oracle)
        self.access_calls, self.score_sizes, self._ens = [], [], {}

    def ensemble(self, seq):
        if seq not in self._ens:
            self._ens[seq] = ar.Ensemble(self.o, seq)
        return self._ens[seq]

    def unpaired_free_energy(self, seqs, masks):
        m = engine.mask_array(masks, len(seqs[0]))
        self.access_calls.append((len(seqs), m.shape[0]))
        return np.array([self.ensemble(s).free_energy(m) for s in seqs])

    opening_energy = engine.Engine.opening_energy

    def score_batch(self, seqs, flags=0):
        self.score_sizes.append(len(seqs))
        return {"Epf": np.array([self.o.pf(s) for s in seqs]), "Emfe": None, "mfe_ss": None, "Ed": None}


class NativeStub(AccessOracleEngine):
    """claims a native loop for Ed-Epf; counts what the driver asks of it"""
    TERM_IDS = {"Ed-Epf": 0}

    def __init__(self, oracle):
        super().__init__(oracle)
        self.native_calls = 0

    def set_motifs(self, motifs):
        pass

    def mc_run(self, *a, **kw):
        self.native_calls += 1
        raise RuntimeError("native loop entered")


def _input(name="hp", ss=HAIRPIN14, region=None):
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr="N" * len(ss), seed_seq=None, alt_sec_struct=None, alt_sec_structs=None,
                           accessible=region)


def _input_file(tmp_path, name, ss, region=None, tail=""):
    f = tmp_path / (name + ".txt")
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss)
                 + (">accessible\n%s\n" % region if region is not None else "") + tail)
    return str(f)


# ------------------------------------------------------------------------------------------------ the input block

def test_block_is_parsed(tmp_path):
    inp = design.read_input(_input_file(tmp_path, "hp", HAIRPIN14, REGION14))
    assert inp.accessible == REGION14 and inp.sec_struct == HAIRPIN14
    assert design.read_input(_input_file(tmp_path, "plain", HAIRPIN14)).accessible is None
    # the block may stand anywhere among the others
    f = tmp_path / "mid.txt"
    f.write_text(">name\nmid\n>accessible\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (REGION14, "N" * 14, HAIRPIN14))
    assert design.read_input(str(f)).accessible == REGION14


@pytest.mark.parametrize("region,ss,word", [("....xxXxxx....", HAIRPIN14, "'X'"), ("....xx(xxx....", HAIRPIN14, "'('"),
                                            ("....xxxxxx...", HAIRPIN14, "13 characters"), ("....xxxxxx.....", HAIRPIN14, "15 characters"),
                                            ("..............", HAIRPIN14, "no 'x'"), ("", HAIRPIN14, "0 characters"),
                                            ("....xxxx&.........", "((((....&....))))", "two-strand")])
def test_bad_blocks_are_refused(tmp_path, region, ss, word):
    with pytest.raises(ValueError) as ex:
        design.read_input(_input_file(tmp_path, "bad", ss, region))
    assert "accessible" in str(ex.value) and word in str(ex.value)
    with pytest.raises(ValueError):                               # an input built by hand is checked when the run is set up
        design.run_design_fast(_input("bad", ss, region), replicas=2, exchange=1, steps=1, engine=object())


# ------------------------------------------------------------------------------------------------ the term

SEQS = ["GGGGAAAAAACCCC", "GCGCAAGAAAGCGC", "GGCAUAAAAAUGCC", "AAAAAAAAAAAAAA"]


@pytest.mark.parametrize("w", (1.0, 2.5))
def test_score_is_the_plain_score_plus_the_weighted_opening_energy(oracle, w):
    eng, hk = AccessOracleEngine(oracle), engine.HostKernels()
    eng.set_targets([HAIRPIN14])
    sf = es.parse_scoring_functions("Ed-Epf:1.0")
    u8 = np.frombuffer("".join(SEQS).encode(), dtype=np.uint8).reshape(len(SEQS), -1)
    motifs = es.parse_motifs("GNRA,-1.5,AAAA,0.25")
    for kw in ({}, dict(motifs=motifs)):
        plain = es.score_arrays(eng, hk, HAIRPIN14, sf, u8, **kw)
        assert not hasattr(plain, "opening_energy") and eng.access_calls == []
        got = es.score_arrays(eng, hk, HAIRPIN14, sf, u8, accessible=design._engine_mask(REGION14), accessible_weight=w, **kw)
        assert eng.access_calls == [(len(SEQS), 1)]                  # one call per batch, M = 1
        eng.access_calls.clear()
        ref = np.array([eng.ensemble(s).free_energy(design._engine_mask(REGION14))[0] - oracle.pf(s) for s in SEQS])
        assert np.abs(got.opening_energy - ref).max() < 1e-12 and (ref >= -1e-12).all() and ref.max() > ar.MIN_EOPEN
        assert np.abs(got.p_unpaired - np.exp(-ref / KT)).max() < 1e-12
        assert np.abs(got.score - (plain.score + w * ref)).max() < 1e-12
        assert (got.score == plain.score + w * got.opening_energy).all()         # the LAST addition, after the motif term
    # the per-replica scorer (run_design): the same sum, record by record, after its own motif term
    for mot in (None, motifs):
        opts = SimpleNamespace(oligo_state="none", pks="off", subopt="off", motifs=mot, param="1999", scoring_f=sf, accessible=None,
                               accessible_weight=w)
        plain = es.ReplicaScorer(_input(), opts, 4, engine=eng).score(SEQS)
        opts.accessible = design._engine_mask(REGION14)
        got = es.ReplicaScorer(_input(region=REGION14), opts, 4, engine=eng).score(SEQS)
        for a, b in zip(plain, got):
            assert not hasattr(a, "opening_energy")
            assert b.scoring_function == a.scoring_function + w * b.opening_energy
            assert abs(b.p_unpaired - math.exp(-b.opening_energy / KT)) < 1e-12
        assert np.abs(np.array([b.opening_energy for b in got]) - ref).max() < 1e-12


def test_weight_must_be_positive(oracle):
    for w in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            design.run_design_fast(_input(region=REGION14), replicas=2, exchange=1, steps=1, engine=AccessOracleEngine(oracle),
                                   accessible_weight=w)


# ------------------------------------------------------------------------------------------------ the drivers

KW = dict(replicas=4, exchange=5, steps=2, seed=3)


def test_records_and_best_carry_the_columns_only_with_the_block(oracle):
    for fast in (True, False):
        res = {}
        for key, region in (("plain", None), ("region", REGION14)):
            eng, inp = AccessOracleEngine(oracle), _input(region=region)
            if fast:
                res[key] = design.run_design_fast(inp, accessible_weight=2.0, engine=eng, native_loop=False, **KW)
            else:                                                 # the per-replica driver, its scorer on the stand-in engine
                opts = SimpleNamespace(oligo_state="none", pks="off", subopt="off", motifs=None, param="1999",
                                       scoring_f=es.parse_scoring_functions("Ed-Epf:1.0"),
                                       accessible=None if region is None else design._engine_mask(region), accessible_weight=2.0)
                res[key] = design.run_design(inp, accessible_weight=2.0, scorer=es.ReplicaScorer(inp, opts, 4, engine=eng), **KW)
        for r in res["plain"]["simulation_data"]:
            assert "opening_energy" not in r and "p_unpaired" not in r
        assert not hasattr(res["plain"]["best"], "opening_energy")
        recs = res["region"]["simulation_data"]
        assert len(recs) == 4 * 3
        for r in recs + [vars(res["region"]["best"])]:
            ens = ar.Ensemble(oracle, r["sequence"])
            ref = ens.free_energy(design._engine_mask(REGION14))[0] - oracle.pf(r["sequence"])
            assert abs(r["opening_energy"] - ref) < 1e-12 and abs(r["p_unpaired"] - math.exp(-ref / KT)) < 1e-12
            plain_score = r["edesired"] - r["Epf"]                      # -sf Ed-Epf:1.0
            assert abs(r["scoring_function"] - (plain_score + 2.0 * ref)) < 1e-9
        assert list(recs[0].keys())[-2:] == ["opening_energy", "p_unpaired"]


def test_a_region_turns_the_native_loop_off(oracle):
    eng = NativeStub(oracle)
    with pytest.raises(RuntimeError, match="native loop entered"):
        design.run_design_fast(_input(), engine=eng, **KW)                 # without the block the native loop is taken ...
    assert eng.native_calls == 1
    eng = NativeStub(oracle)
    res = design.run_design_fast(_input(region=REGION14), engine=eng, native_loop=True, **KW)
    assert eng.native_calls == 0 and res["used_native_loop"] is False      # ... with it never, whatever the caller asks
    assert eng.access_calls == [(4, 1)] * (1 + KW["steps"] * KW["exchange"])


def test_batch_eligibility_and_the_lock_step_batch(oracle):
    assert design.batch_eligible(_input()) and not design.batch_eligible(_input(region=REGION14))
    with pytest.raises(ValueError, match="accessible"):
        design.run_puzzle_batch([_input(), _input("r", region=REGION14)], engine=object(), **dict(KW, steps=1))


# ------------------------------------------------------------------------------------------------ the command line

REAL_FAST, REAL_BATCH = design.run_design_fast, design.run_puzzle_batch


def _run_cli(monkeypatch, tmp_path, oracle, extra, source, outdir="out", spy=None):
    """the command line on the stand-in engine; spy collects (driver name, inputs' names, the keywords the command line passed)"""
    eng = AccessOracleEngine(oracle)
    spy = [] if spy is None else spy

    def fast(inp, **kw):
        spy.append(("fast", [inp.name], kw))
        return REAL_FAST(inp, engine=eng, **dict(kw, native_loop=False))

    def batch(inputs, **kw):
        spy.append(("batch", [i.name for i in inputs], kw))
        return REAL_BATCH(inputs, engine=eng, **dict(kw, native_loop=False))

    monkeypatch.setattr(design, "run_design_fast", fast)
    monkeypatch.setattr(design, "run_puzzle_batch", batch)
    out = tmp_path / outdir
    design.main(source + ["-R", "4", "-e", "5", "-s", "2", "-seed", "3", "-r", "6", "-o", str(out)] + extra)
    return eng, out


def _one(out, suffix, prefix=""):
    (p,) = [p for p in out.iterdir() if p.name.endswith(suffix) and p.name.startswith(prefix)]
    return p


def test_results_csv_carries_the_columns_only_with_the_block(monkeypatch, tmp_path, oracle):
    _, out = _run_cli(monkeypatch, tmp_path, oracle, ["--accessible-weight", "2.5"], ["-f", _input_file(tmp_path, "hp", HAIRPIN14, REGION14)])
    rows = list(csv.DictReader(open(_one(out, "_results.csv"))))
    assert rows and list(rows[0].keys())[-2:] == ["opening_energy", "p_unpaired"]
    for r in rows:
        ref = ar.Ensemble(oracle, r["sequence"]).free_energy(design._engine_mask(REGION14))[0] - oracle.pf(r["sequence"])
        assert abs(float(r["opening_energy"]) - ref) < 1e-9
        assert abs(float(r["scoring_function"]) - (float(r["edesired"]) - float(r["Epf"]) + 2.5 * ref)) < 1e-9
    assert "opening_energy" in open(_one(out, "_traj.csv")).readline()
    _, out = _run_cli(monkeypatch, tmp_path, oracle, ["--accessible-weight", "2.5"], ["-f", _input_file(tmp_path, "pl", HAIRPIN14)], "out2")
    assert "opening_energy" not in open(_one(out, "_results.csv")).readline()
    assert "opening_energy" not in open(_one(out, "_traj.csv")).readline()


def test_set_with_a_region_among_plain_inputs_designs_all(monkeypatch, tmp_path, oracle):
    files = [_input_file(tmp_path, "pa", HAIRPIN14), _input_file(tmp_path, "rg", HAIRPIN14, REGION14),
             _input_file(tmp_path, "pb", "(((....)))....")]
    spy = []
    _, out = _run_cli(monkeypatch, tmp_path, oracle, ["--accessibility", "4"], ["--set"] + files, "set", spy)
    batches = [names for kind, names, _ in spy if kind == "batch"]
    assert [names for kind, names, _ in spy if kind == "fast"] == [["rg"]]
    assert batches == [["pa", "pb"]]                               # the plain ones in lock-step, the region through its own driver
    for name, cols in (("pa", False), ("rg", True), ("pb", False)):
        assert ("opening_energy" in open(_one(out, "_results.csv", name + "_")).readline()) is cols
        rows = list(csv.DictReader(open(_one(out, "_accessibility.csv", name + "_"))))
        n_seq = len(list(csv.DictReader(open(_one(out, "_results.csv", name + "_")))))
        assert len(rows) == n_seq * (14 - 4 + 1 + int(cols))
        assert (rows[0]["kind"] == "region") is cols


def test_accessibility_report(monkeypatch, tmp_path, oracle):
    W = 5
    for region in (REGION14, None):
        eng, out = _run_cli(monkeypatch, tmp_path, oracle, ["--accessibility", str(W)],
                            ["-f", _input_file(tmp_path, "hp", HAIRPIN14, region)], "out_" + str(region is None))
        res_file, acc_file = _one(out, "_results.csv"), _one(out, "_accessibility.csv")
        assert acc_file.name == res_file.name.replace("_results.csv", "_accessibility.csv")
        reported = [r["sequence"] for r in csv.DictReader(open(res_file))]
        per = 14 - W + 1 + (region is not None)
        # one engine call per chunk of max_R sequences, all windows (+ the region) as its masks; Epf from the chunk's score batch
        assert eng.access_calls[-(-(-len(reported) // eng.max_R)):] == [(min(eng.max_R, len(reported) - k), per)
                                                                        for k in range(0, len(reported), eng.max_R)]
        assert sum(eng.score_sizes) == len(reported) and max(eng.score_sizes) <= eng.max_R
        rows = list(csv.DictReader(open(acc_file)))
        assert tuple(rows[0].keys()) == outputs.ACCESSIBILITY_COLUMNS == ("sequence", "kind", "start", "end", "opening_energy", "p_unpaired")
        assert [r["sequence"] for r in rows] == [s for s in reported for _ in range(per)]
        for seq in reported:
            mine = [r for r in rows if r["sequence"] == seq]
            ens = ar.Ensemble(oracle, seq)
            if region is not None:
                first = mine.pop(0)
                ref = ens.free_energy(design._engine_mask(region))[0] - oracle.pf(seq)
                assert (first["kind"], first["start"], first["end"]) == ("region", "5", "10")
                assert float(first["opening_energy"]) == round(ref, 3) and float(first["p_unpaired"]) == round(math.exp(-ref / KT), 3)
            ref = ens.free_energy(ar.window_masks(14, W)) - oracle.pf(seq)
            assert [(r["kind"], int(r["start"]), int(r["end"])) for r in mine] == [("window", a, a + W - 1) for a in range(1, 14 - W + 2)]
            for r, e in zip(mine, ref):                                # rounded as _structures.csv is: three decimals
                assert float(r["opening_energy"]) == round(float(e), 3) and float(r["p_unpaired"]) == round(math.exp(-e / KT), 3)


def test_flag_parsing(monkeypatch, tmp_path, capsys):
    one = _input_file(tmp_path, "hp", HAIRPIN14, REGION14)
    two = _input_file(tmp_path, "two", "((((....&....))))")

    class Started(Exception):
        pass

    def started(*a, **k):
        raise Started()

    monkeypatch.setattr(design, "run_design_fast", started)
    monkeypatch.setattr(design, "run_design", started)
    monkeypatch.setattr(design, "run_puzzle_set", started)
    o = str(tmp_path / "o")
    for argv, word in ((["-f", one, "--accessibility", "4"], "give -o"), (["-f", one, "--accessibility", "0", "-o", o], "W >= 1"),
                       (["-f", one, "--accessibility", "-3", "-o", o], "W >= 1"), (["-f", one, "--accessibility", "x", "-o", o], "invalid int"),
                       (["-f", two, "--accessibility", "4", "-o", o], "two-strand"), (["--set", one, two, "--accessibility", "4", "-o", o], "two-strand"),
                       (["-f", one, "--accessible-weight", "0"], "W > 0"), (["-f", one, "--accessible-weight", "-1"], "W > 0")):
        with pytest.raises(SystemExit) as ex:
            design.main(argv)
        assert ex.value.code == 2 and word in capsys.readouterr().err, argv
    for argv in (["-f", one], ["--set", one, one]):
        with pytest.raises(Started):
            design.main(argv + ["--accessibility", "4", "--accessible-weight", "0.5", "-o", o])


def test_without_block_and_flags_the_files_are_what_they_were(monkeypatch, tmp_path, oracle):
    """a seeded run without the block: the command line as it was, and the same call with the new keywords spelled out at their
    defaults, write the same files byte for byte (clock and time stamp held still)"""
    monkeypatch.setattr(design, "time", SimpleNamespace(time=lambda: 1000.0, strftime=lambda *a: "20260101.000000"))
    plain = _input_file(tmp_path, "hp", HAIRPIN14)
    spy = []
    _, a = _run_cli(monkeypatch, tmp_path, oracle, [], ["-f", plain], "a", spy)
    _, b = _run_cli(monkeypatch, tmp_path, oracle, ["--accessible-weight", "1.0"], ["-f", plain], "b", spy)
    assert len(spy) == 2 and all("accessible_weight" not in kw for _, _, kw in spy)       # the driver's keywords are what they were
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and len(names) == 6 and not [n for n in names if "accessib" in n]
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    # ... and the API: the keyword at its default against the keyword left out
    kw = dict(KW, native_loop=False)
    x = REAL_FAST(_input(), engine=AccessOracleEngine(oracle), **kw)
    y = REAL_FAST(_input(), engine=AccessOracleEngine(oracle), accessible_weight=1.0, **kw)
    assert x["simulation_data"] == y["simulation_data"] and vars(x["best"]) == vars(y["best"]) and x["stats"].keys() == y["stats"].keys()
