"""design.ensemble_report on a two-strand design, with a stand-in engine (no GPU) that draws with numpy from the exact co-fold
distribution of each pair (tests/cofold_sampling_ref.py): one call, the '&' kept in every structure compared and written, counts
adding up to S, Epf = FAB.  And the one-strand report: its file is byte for byte what the report wrote before two strands were
accepted."""
import csv
import io
from collections import Counter
from types import SimpleNamespace

import numpy as np

from desirna_amd import design, outputs
from desirna_amd import engine as _engine
from tests import cofold_sampling_ref as cr
from tests import sampling_ref as sr

S = 200
PAIRS = ["ACAGAAUU&GUCA", "UAGAUUAC&AGAA"]
TARGET = "((......&..))"      # 8+4: two pairs across the nick
ONE = ["GGGGAAAACCCC", "GGGAAAACCCGC"]
ONE_TARGET = "((((....))))"


class StandIn:
    """counted samplers over exact distributions; the two-strand one returns what Engine.cofold_sample_structures returns"""

    def __init__(self, oracle):
        self.o = oracle
        self.calls = []

    def _draw(self, dist, S, seed):
        keys = sorted(dist)
        p = np.array([dist[k] for k in keys])
        return [keys[k] for k in np.random.default_rng(seed).choice(len(keys), S, p=p / p.sum())]

    def cofold_sample_structures(self, seqs, S, seed=0):
        self.calls.append(("two", list(seqs), S, seed))
        out = [self._draw(cr.exact_distribution(self.o, p)[0], S, seed + r) for r, p in enumerate(seqs)]
        E = np.array([[self.o.eval_structure(p.replace("&", ""), s.replace("&", ""), p.index("&")) for s in row]
                      for p, row in zip(seqs, out)], dtype=np.int32)
        return out, E, np.array([self.o.cofold_pf(p) for p in seqs])

    def sample_structures(self, seqs, S, seed=0):
        self.calls.append(("one", list(seqs), S, seed))
        out = [self._draw(sr.exact_distribution(self.o, q), S, seed + r) for r, q in enumerate(seqs)]
        E = np.array([[self.o.eval_structure(q, s) for s in row] for q, row in zip(seqs, out)], dtype=np.int32)
        return out, E, np.array([self.o.pf(q) for q in seqs])


def _inp(target):
    return SimpleNamespace(name="x", sec_struct=target, seq_restr="N" * len(target), seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


def test_two_strand_report(oracle):
    assert len(TARGET) == len(PAIRS[0]) and TARGET.index("&") == PAIRS[0].index("&")
    eng = StandIn(oracle)
    rows = design.ensemble_report(eng, {"reported": PAIRS, "simulation_data": []}, _inp(TARGET), S, top=3, seed=5)
    assert eng.calls == [("two", PAIRS, S, 5)]                            # one call, the two-strand sampler
    text = outputs.ensemble_csv_text(rows)
    got = list(csv.DictReader(io.StringIO(text)))
    assert tuple(got[0].keys()) == outputs.ENSEMBLE_COLUMNS
    for r, pair in enumerate(PAIRS):
        mine = [x for x in got if x["sequence"] == pair]
        kinds = [x["kind"] for x in mine]
        ntop = kinds.count("top")
        assert 1 <= ntop <= 3 and kinds == ["top"] * ntop + ["target", "other"]
        top, target, other = mine[:ntop], mine[ntop], mine[ntop + 1]
        drawn = Counter(eng._draw(cr.exact_distribution(oracle, pair)[0], S, 5 + r))
        for x in top + [target]:
            assert x is target or cr.well_formed(pair, x["structure"])
            # the '&' is in every structure row, where the pair has it
            assert x["structure"].count("&") == 1 and x["structure"].index("&") == pair.index("&")
            assert int(x["count"]) == drawn.get(x["structure"], 0)
            assert abs(float(x["Epf"]) - oracle.cofold_pf(pair)[3]) < 1e-3   # Epf = FAB
        assert target["structure"] == TARGET and float(target["mcc"]) == 0.0
        for x in top:
            e = oracle.eval_structure(pair.replace("&", ""), x["structure"].replace("&", ""), pair.index("&")) / 100.0
            assert abs(float(x["energy"]) - e) < 1e-9
        in_top = TARGET in [x["structure"] for x in top]
        assert sum(int(x["count"]) for x in top) + int(other["count"]) + (0 if in_top else int(target["count"])) == S
        assert [x["structure"] for x in top] == sorted(drawn, key=lambda s: (-drawn[s], s))[:ntop]


def _rows_before(engine, seqs, target, S, top, seed):
    """the one-strand report as it was written before two strands were accepted"""
    ss, E, Epf = engine.sample_structures(seqs, S, seed)
    hk = _engine.HostKernels()
    rows = []
    for r, seq in enumerate(seqs):
        cnt = Counter(ss[r])
        energy = {s: int(E[r][k]) / 100.0 for k, s in enumerate(ss[r])}
        first = sorted(cnt, key=lambda s: (-cnt[s], s))[:top]
        listed = first + [target]
        mcc = 1.0 - hk.simscore(target, np.frombuffer("".join(listed).encode("ascii"), dtype=np.uint8).reshape(len(listed), -1))[0]
        row = lambda kind, rank, s, c, e, m: dict(sequence=seq, Epf=float(Epf[r]), kind=kind, rank=rank, structure=s, count=int(c),
                                                  frequency=c / S, energy=e, mcc=m)
        for k, s in enumerate(first):
            rows.append(row("top", k + 1, s, cnt[s], energy[s], float(mcc[k])))
        e_t = energy.get(target)
        rows.append(row("target", "", target, cnt.get(target, 0), "" if e_t is None else float(e_t), float(mcc[-1])))
        rows.append(row("other", "", "", S - sum(cnt[s] for s in set(first) | {target}), "", ""))
    return rows


def test_one_strand_rows_unchanged(oracle):
    eng = StandIn(oracle)
    rows = design.ensemble_report(eng, {"reported": ONE, "simulation_data": []}, _inp(ONE_TARGET), S, top=4, seed=9)
    assert eng.calls == [("one", ONE, S, 9)]
    assert outputs.ensemble_csv_text(rows) == outputs.ensemble_csv_text(_rows_before(StandIn(oracle), ONE, ONE_TARGET, S, 4, 9))
