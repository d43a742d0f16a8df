"""Sequence motifs (-motifs) on the host path, no GPU: the native matcher (drna_motif_score_batch) against Python's ``re`` on the
regular expressions of energy_scores.parse_motifs, the parser's errors, score_arrays(motifs=...) against ReplicaScorer.score,
the three drivers against each other on oracle-backed stand-in engines, and the command line."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

from desirna_amd import design, engine
from desirna_amd import energy_scores as es
from tests.test_design_driver import ETE1, OracleEngine
from tests.test_nd_native_host import HAIRPIN14, NdCoEngine
from tests.test_oa_native_host import OaEngine, _same_walk
from tests.test_puzzle_set_host import RaggedOracleEngine, _same_run

MOTIFS = "GNRA,-2,GGGG,3"
BAD = ["GNRA,-2,GGGG", "GNXA,1", "gnra,1", "GNRA,x"]          # an odd count, an unknown letter, lower case, a value that is no float
CLASSES = es.MOTIF_LETTERS


@pytest.fixture(scope="module")
def hk():
    return engine.HostKernels()


def _u8(seqs):
    return np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1)


def _term(parsed, seq):
    """the reference's sum: 0 + the values of the motifs found, in dict order"""
    return es.score_motifs(seq, SimpleNamespace(motifs=parsed))


def _same_bytes(got, want):
    assert got.dtype == np.float64 and got.tobytes() == np.array(want, dtype=np.float64).tobytes(), (got, want)


def _text(pairs):
    return ",".join("%s,%r" % (k, v) for k, v in pairs)


# ---- 1. the matcher

def _motif_near(rng, seq):
    """a motif made from a stretch of `seq`: every letter replaced by a class that holds it, now and then by one that does not"""
    n = rng.randint(0, min(70, len(seq)))
    at = rng.randint(0, len(seq) - n)
    out = []
    for ch in seq[at:at + n]:
        pool = [k for k, v in CLASSES.items() if (ch in v) != (rng.random() < 0.02)]
        out.append(rng.choice(pool))
    return "".join(out)


def test_matcher_equals_python_re_on_random_sequences_and_motif_sets(hk):
    rng = random.Random(20240611)
    seqs = ["".join(rng.choice("ACGU") for _ in range(rng.randint(1, 80))) for _ in range(2000)]
    by_len = {}
    for s in seqs:
        by_len.setdefault(len(s), []).append(s)
    assert min(by_len) == 1 and max(by_len) == 80
    long_seqs = [s for s in seqs if len(s) >= 66]
    sets = []
    for k in range(200):
        pairs = []
        for _ in range(rng.randint(1, 5)):
            kind = rng.random()
            if kind < 0.1:
                key = ""
            elif kind < 0.4:
                key = "".join(rng.choice(list(CLASSES)) for _ in range(rng.randint(0, 70)))
            elif kind < 0.6:
                key = _motif_near(rng, rng.choice(long_seqs))
            else:
                key = _motif_near(rng, rng.choice(seqs))[:rng.randint(1, 12)]
            pairs.append((key, rng.choice([-1, 1]) * round(rng.uniform(0.01, 9), rng.randint(0, 6))))
        sets.append(pairs)
    sets[0] = [("A" * 65, 1.5), ("N" * 64, -0.25), ("W" * 70, 3.0), ("", 0.125)]          # around the 64-letter bound
    keys = [k for pairs in sets for k, _ in pairs]
    assert set("".join(keys)) == set(CLASSES) and len(CLASSES) == 16
    assert "" in keys and max(map(len, keys)) == 70 and any(v < 0 for p in sets for _, v in p) and any(v > 0 for p in sets for _, v in p)
    hits = {True: [0, 0], False: [0, 0]}            # [motif longer than 64][found or not]: every branch of the matcher decided both ways
    for pairs in sets:
        parsed = es.parse_motifs(_text(pairs))
        assert [v for _, v in parsed.values()] == [dict(pairs)[k] for k in parsed]
        for key, (rx, _) in parsed.items():
            for s in (long_seqs if len(key) > 64 else rng.sample(seqs, 20)):
                hits[len(key) > 64][bool(rx.search(s))] += 1
        for L, group in by_len.items():
            _same_bytes(hk.motif_score(parsed, _u8(group)), [_term(parsed, s) for s in group])
    assert all(min(h) > 0 for h in hits.values()), hits


def test_matcher_fixed_cases(hk):
    one = lambda motifs, seq: float(hk.motif_score(motifs, _u8([seq]))[0])
    assert one([("GNRA", -2.0)], "GAAACCCC") == -2.0                  # a hit at the first position
    assert one([("GNRA", -2.0)], "CCCCGCGA") == -2.0                  # ... at the last
    assert one([("GNRA", -2.0)], "CCCGCGAC") == -2.0
    assert one([("GNRA", -2.0)], "CCCGCGCC") == 0.0
    assert one([("ACAC", 1.0)], "GACACACG") == 1.0                    # overlapping occurrences count once
    assert one([("AAUAA", 1.0)], "AAUAAUAA") == 1.0
    assert one([("AAUAAC", 1.0)], "AAUAAUAAC") == 1.0                 # a hit that starts inside a failed attempt
    assert one([("ACGUA", 1.0)], "ACGU") == 0.0                       # longer than the sequence
    assert one([("A" * 65, 1.0)], "A" * 64) == 0.0 and one([("A" * 65, 1.0)], "C" + "A" * 65) == 1.0
    assert one([("N" * 64, 1.0)], "A" * 63) == 0.0 and one([("N" * 64, 1.0)], "ACGU" * 16) == 1.0
    # T is a letter of its own: the motif T finds it, U and N do not
    assert [one([(m, 1.0)], "AATAA") for m in ("T", "U", "N", "ATA", "ANA", "AUA", "NN", "NNN")] == [1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    assert one([("T", 1.0)], "AAUAA") == 0.0
    # two strands: the '&' is in no class, so nothing matches across the nick; each strand alone is searched
    assert one([("GGCC", 1.0)], "AAGG&CCAA") == 0.0 and one([("GGNCC", 1.0)], "AAGG&CCAA") == 0.0
    assert one([("AAGG", 1.0), ("CCAA", 2.0), ("GGCC", 4.0)], "AAGG&CCAA") == 3.0
    assert one([("", 0.5)], "A") == 0.5 and one([], "ACGU") == 0.0 and one(None, "ACGU") == 0.0
    # a repeated key keeps its first position and takes its last value: ((0 - 1e16) + 1e16) + 1, not (1e16 + 1) - 1e16
    rep = [("GG", 7.0), ("AA", 1e16), ("CC", 1.0), ("GG", -1e16)]
    parsed = es.parse_motifs(_text(rep))
    assert list(parsed) == ["GG", "AA", "CC"] and parsed["GG"][1] == -1e16
    assert one(rep, "GGAACC") == one(parsed, "GGAACC") == _term(parsed, "GGAACC") == 1.0
    assert one(rep, "GGAAC") == 0.0 and one(rep, "CCAA") == 1e16 + 1.0
    for bad in ("GNXA", "gnra", "GN&A", "GN A", "GÅ"):
        with pytest.raises(engine.EngineError) as err:
            hk.motif_score([("GGGG", 1.0), (bad, 1.0)], _u8(["ACGU"]))
        assert err.value.code == -1 and "drna_motif_score_batch" in str(err.value)


# ---- 2. the parser

def test_parse_motifs_and_its_errors(tmp_path, capsys):
    assert es.parse_motifs("") == {}
    p = es.parse_motifs("GNRA,-2,GGGG,3,,0.5")
    assert list(p) == ["GNRA", "GGGG", ""] and [v for _, v in p.values()] == [-2.0, 3.0, 0.5]
    assert p["GNRA"][0].pattern == "G[ACGU][AG]A" and p[""][0].search("ACGU")
    assert sorted(CLASSES) == sorted("ACGTUWSMKRYBDHVN")
    f = tmp_path / "d.txt"
    f.write_text(">name\nx\n>seq_restr\n%s\n>sec_struct\n%s\n" % ("N" * 14, HAIRPIN14))
    for bad in BAD:
        with pytest.raises(ValueError, match="Something is wrong with your motifs"):
            es.parse_motifs(bad)
        with pytest.raises(ValueError):
            design.run_design_fast(design.read_input(str(f)), replicas=2, exchange=1, steps=1, engine=object(), native_loop=False, motifs=bad)
        for argv in (["-f", str(f)], ["--set", str(f), str(f)], ["-f", str(f), "--python-host"]):
            with pytest.raises(SystemExit):
                design.main(argv + ["-motifs", bad])
            assert "Something is wrong with your motifs" in capsys.readouterr().err


# ---- 3. score_arrays(motifs=...) against ReplicaScorer.score

def _opts(state, nd, motifs):
    return SimpleNamespace(oligo_state=state, pks="off", subopt=nd, motifs=motifs, param="1999",
                           scoring_f=es.parse_scoring_functions("Ed-Epf:1.0"))


@pytest.mark.parametrize("case", ["one_strand", "oa", "nd", "two_strands"])
def test_score_arrays_with_motifs_equals_replica_scorer(oracle, example_inputs, hk, case):
    across = "CCGG"
    if case == "two_strands":
        ex = example_inputs["RNA_RNA_complex_design_input"]
        ss = ex["sec_struct"][0]
        prob = design.DesignProblem(ss, ex["seq_restr"][0])
        rng = random.Random(4)
        seqs = [prob.initial_sequence(rng) for _ in range(4)]
        cut = ss.index("&")
        across = seqs[0][cut - 4:cut] + seqs[0][cut + 1:cut + 5]              # occurs across the nick of seqs[0], and nowhere else
        assert all(across not in s.split("&")[0] and across not in s.split("&")[1] for s in seqs) and across in seqs[0].replace("&", "")
        state, nd, mk = "heterodimer", "off", NdCoEngine
    else:
        ss = HAIRPIN14
        seqs = ["GGGGAAAAAACCCC", "GCGCAAAAAAGCGC", "CUCUUUUUUUAGAG", "CCCCUUUUUUGGGG", "CCGGAUAUAACCGG"]
        state, nd, mk = "avoid" if case == "oa" else "none", "on" if case == "nd" else "off", OaEngine
    parsed = es.parse_motifs(MOTIFS + ",,0.5,%s,0.25" % across)
    inp = SimpleNamespace(name=case, sec_struct=ss, seq_restr="N" * len(ss), seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    want = es.ReplicaScorer(inp, _opts(state, nd, parsed), len(seqs), engine=mk(oracle)).score(seqs)
    plain = es.ReplicaScorer(inp, _opts(state, nd, None), len(seqs), engine=mk(oracle)).score(seqs)
    eng = mk(oracle)
    eng.set_targets([ss.replace("&", "")])
    args = (eng, hk, ss, es.parse_scoring_functions("Ed-Epf:1.0"), _u8(seqs), state, "off", nd == "on")
    got = es.score_arrays(*args, self_dimer=case == "oa", motifs=parsed)
    terms = [_term(parsed, s) for s in seqs]
    assert len(set(terms)) > 1, terms
    if case != "two_strands":
        assert len(set(terms)) > 2 and 0.5 in terms and 0.75 in terms, terms            # 0.5: the empty motif alone
    for k, s in enumerate(seqs):
        assert float(got.score[k]) == want[k].scoring_function == plain[k].scoring_function + terms[k], (case, s)
        assert vars(es.record(got, k)) == vars(want[k]), (case, s)          # no column of its own
    if case == "nd":
        assert any(sc.mcc == 0 and sc.esubopt_minus_Epf != 0 for sc in want)          # a solved candidate took the -nd branch
    # motifs=None, and an empty set, are the call without the keyword
    base = es.score_arrays(*args, self_dimer=case == "oa")
    for kw in (dict(motifs=None), dict(motifs={})):
        off = es.score_arrays(*args, self_dimer=case == "oa", **kw)
        assert sorted(vars(off)) == sorted(vars(base))
        for name, a in vars(base).items():
            b = getattr(off, name)
            assert (a.tobytes() == b.tobytes() and a.dtype == b.dtype) if isinstance(a, np.ndarray) else a == b, name
    assert [float(x) for x in base.score] == [sc.scoring_function for sc in plain]


# ---- 4. the drivers

def _inp(name, ss):
    """a hairpin whose loop holds no G: the initial sequence's loop is UAAAAA, so GNRA occurs when the stem ends in G (the seeds
    below were picked with the oracle: their records hold terms of 0, -2 and 3)"""
    return SimpleNamespace(name=name, sec_struct=ss, seq_restr=ss.replace("(", "N").replace(")", "N").replace(".", "H"), seed_seq=None,
                           alt_sec_struct=None, alt_sec_structs=None)


def _mixed_terms(records, parsed):
    """the motif term of every recorded sequence: non-zero for some, zero for others (otherwise the case shows nothing), and
    it is in the score: -sf is Ed-Epf:1.0, so score = (Ed - Epf) + term"""
    terms = [_term(parsed, r["sequence"]) for r in records]
    assert any(t != 0 for t in terms) and any(t == 0 for t in terms), sorted(set(terms))
    for r, t in zip(records, terms):
        assert r["scoring_function"] == r["edesired_minus_Epf"] + t
    return terms


def test_python_and_fast_driver_walk_the_same_trajectory_with_motifs(oracle):
    inp, kw = _inp("hairpin14", HAIRPIN14), dict(replicas=6, exchange=15, steps=4, seed=5)
    parsed = es.parse_motifs(MOTIFS)
    ea, eb = OaEngine(oracle), OaEngine(oracle)
    a = design.run_design(inp, scorer=es.ReplicaScorer(inp, _opts("none", "off", parsed), kw["replicas"], engine=ea), motifs=MOTIFS, **kw)
    b = design.run_design_fast(inp, engine=eb, native_loop=False, motifs=MOTIFS, **kw)
    assert not b["used_native_loop"]
    _same_walk(a, b, oa=False)
    for x, y in zip(a["simulation_data"], b["simulation_data"]):
        assert x["scoring_function"] == y["scoring_function"] and list(x) == list(y)
    _mixed_terms(b["simulation_data"], parsed)
    # run_design builds its scorer from the keyword as well (here: the options it hands to it), and the parsed dict is the text
    assert design._setup(inp, 2, 1, 1, 10.0, 150.0, "Ed-Epf:1.0", 1, False, None, None, motifs=MOTIFS).opts.motifs.keys() == parsed.keys()
    c = design.run_design_fast(inp, engine=OaEngine(oracle), native_loop=False, motifs=parsed, **kw)
    assert c["simulation_data"] == b["simulation_data"]
    # without motifs the walk is another one
    d = design.run_design_fast(inp, engine=OaEngine(oracle), native_loop=False, **kw)
    assert [r["sequence"] for r in d["simulation_data"]] != [r["sequence"] for r in b["simulation_data"]]


def test_puzzle_batch_equals_every_puzzle_alone_with_motifs(oracle):
    puzzles = [_inp("hairpin14", HAIRPIN14), _inp("eteV1_01", ETE1)]
    kw = dict(replicas=4, exchange=10, seed=5, steps=3, native_loop=False, motifs=MOTIFS)
    eng = RaggedOracleEngine(oracle)
    got = design.run_puzzle_batch(puzzles, engine=eng, **kw)
    parsed = es.parse_motifs(MOTIFS)
    for inp, a in zip(puzzles, got):
        _same_run(a, design.run_design_fast(inp, engine=OracleEngine(oracle), **kw))
        _mixed_terms(a["simulation_data"], parsed)
    assert eng.ragged_calls == 1 + 3 * 10 and eng.rect_calls == 0


# ---- 5. the command line

def test_cli_hands_the_parsed_motifs_to_every_driver(monkeypatch, tmp_path, capsys):
    files = []
    for name, ss in (("a", HAIRPIN14), ("b", ETE1)):
        f = tmp_path / (name + ".txt")
        f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (name, "N" * len(ss), ss))
        files.append(str(f))
    seen = []

    def fake(which):
        def run(inp, **kw):
            seen.append((which, kw))
            best = SimpleNamespace(sequence="A" * 14, mfe_ss="." * 14, Epf=0.0, edesired=0.0, mcc=1.0, scoring_function=0.0)
            res = {"best": best, "solved": False, "steps": 0, "stats": {"scored": 0, "elapsed_s": 0.0}}
            return [res for _ in inp] if which == "batch" else res
        return run

    for which, name in (("python", "run_design"), ("fast", "run_design_fast"), ("batch", "run_puzzle_batch")):
        monkeypatch.setattr(design, name, fake(which))
    design.main(["-f", files[0], "-motifs", MOTIFS])
    design.main(["-f", files[0], "--motif_sequences", MOTIFS, "--python-host"])
    design.main(["-f", files[0], "-motifs", MOTIFS, "-acgu", "on", "-acgu_content", "25,25,25,25"])
    design.main(["--set"] + files + ["-motifs", MOTIFS])
    assert [w for w, _ in seen] == ["fast", "python", "python", "batch"]
    for _, kw in seen:
        assert list(kw["motifs"]) == ["GNRA", "GGGG"] and [v for _, v in kw["motifs"].values()] == [-2.0, 3.0]
        assert kw["motifs"]["GNRA"][0].search("CCGAGACC")
    with_flag = [set(kw) for _, kw in seen]
    seen.clear()
    design.main(["-f", files[0]])
    design.main(["-f", files[0], "--python-host"])
    design.main(["-f", files[0], "-acgu", "on", "-acgu_content", "25,25,25,25"])
    design.main(["--set"] + files)
    assert [w for w, _ in seen] == ["fast", "python", "python", "batch"]
    assert all("motifs" not in kw for _, kw in seen)                         # without the flag no driver sees the keyword
    assert [set(kw) | {"motifs"} for _, kw in seen] == with_flag              # ... and the flag adds nothing else
    # a puzzle stays eligible for the lock-step batch with motifs
    assert design.batch_eligible(_inp("a", HAIRPIN14), motifs=es.parse_motifs(MOTIFS)) and design.batch_eligible(_inp("a", HAIRPIN14))
    capsys.readouterr()
