"""The sequence pairs on which the GPU's ranked co-fold structures are compared with the emulated kernel byte for byte, and the
record of the emulation's answers (tests/golden/cofold_kbest_emulated.json).

The emulation of one pair takes seconds (its time goes into the rendezvous of 64 OS threads), so the GPU test reads the record;
tests/test_cofold_kbest_emulated.py recomputes every entry and fails when the record is not what the kernel source in the tree
gives.  ``python -m tests.cofold_kbest_cases`` rewrites the record.  A plain helper module (no fixtures, no pytest configuration)."""
import csv
import gzip
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(_HERE, "golden", "cofold_kbest_emulated.json")
KS = (4, 8)               # the two kernel instances; a call with K <= 4 is the cut of the 4-list
NT = 64


def _rand(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def pairs():
    """the 60 enumeration pairs (4 - 8 nt per strand), three rows each of the golden two-strand shapes 17+18 and 17+17, the
    bounds 1+1, 1+35, 35+1, and one X&X"""
    from tests.test_cofold_subopt_emulated import _enumeration_cases
    out = _enumeration_cases()
    with gzip.open(os.path.join(_HERE, "golden", "traj_golden.csv.gz"), "rt") as fh:
        rows = list(csv.DictReader(fh))
    for run in ("RNA_RNA_complex_design_input", "Homodimer_design_input"):
        out += [r["sequence"] for r in rows if r["run"] == run][5:200:65]
    rng = np.random.default_rng(31)
    x = _rand(rng, 13, "GGCCAU")
    out += ["G&C", "A&A", "G&" + _rand(rng, 35), _rand(rng, 35) + "&C", _rand(rng, 1) + "&" + _rand(rng, 35),
            _rand(rng, 35) + "&" + _rand(rng, 1), x + "&" + x]
    return out


def emulate(seqs):
    """{K: [[energies, strings], ...]} of the emulated cofold_kbest_kernel<64, K>, one pair per job"""
    from tests.emu.emu_cofold_kbest import cofold_kbest_many
    out = {}
    for K in KS:
        got = cofold_kbest_many([(s, K, NT) for s in seqs])
        assert all(st == 0 for _, _, st in got)
        out[K] = [[E, ss] for E, ss, _ in got]
    return out


def load():
    """(pairs, {K: [[energies, strings], ...]}) of the record"""
    with open(RECORD) as fh:
        d = json.load(fh)
    return d["pairs"], {K: d["K%d" % K] for K in KS}


if __name__ == "__main__":
    seqs = pairs()
    got = emulate(seqs)
    with open(RECORD, "w") as fh:
        json.dump({"pairs": seqs, **{"K%d" % K: got[K] for K in KS}}, fh, indent=0)
        fh.write("\n")
    print(RECORD, os.path.getsize(RECORD), "bytes,", len(seqs), "pairs")
