"""The four kernels of the auxiliary folds in their ragged form (a shuffled workgroup list, one concatenated sequence buffer, the
pitch and slot size of the longest length, per-sequence targets) against their uniform form, one launch per length: the same
bytes.  The kernel sources are compiled unmodified for the CPU (tests/emu/emu_ragged_aux.cpp), workgroups of 64 and 128 threads.

The workspace slots of the emulation start filled with 0xFF bytes (NaN / -1), so a fold that read a cell it had not written would
show in either form; the slot-reuse case sends three lengths through one slot, longest first, and expects the values of the
folds alone.  All emulation jobs of the module run once, side by side in worker processes."""
import numpy as np
import pytest

from tests.emu import emu_ragged_aux

ST_OK, ST_BAD_CHAR = 0, 1
NTS = (64, 128)
GOLD = {12: "eteV1_08", 36: "eteV1_03", 40: "eteV1_65", 42: "eteV1_20", 80: "eteV1_52"}


def _rand(rng, n):
    return "".join(rng.choice(list("ACGU"), size=n))


@pytest.fixture(scope="module")
def cases(eterna_solutions):
    sol = {r["name"].replace(".txt", ""): (r["sequence"], r["structure"]) for r in eterna_solutions}
    rng = np.random.default_rng(20)
    seq, tgt = {}, {}
    for n, name in GOLD.items():
        seq[n], tgt[n] = sol[name]
        assert len(seq[n]) == n
    seq[1], tgt[1] = "G", "."
    seq[4], tgt[4] = "GAAC", "...."
    seq[5], tgt[5] = "GAAAC", "(...)"
    seq[79], tgt[79] = seq[80][:79], None
    bad = seq[12][:6] + "X" + seq[12][7:]
    # (kind, [(sequence, target)] in caller order); the bad letter sits in the middle of the fused kernel's batch
    sets = {
        "edef_lds": [(seq[n], tgt[n]) for n in (1, 4, 5)] + [(bad, tgt[12])] + [(seq[n], tgt[n]) for n in (12, 36, 40)],
        "edef_general": [(seq[n], tgt[n]) for n in (5, 12, 42)],
        "subopt_lds": [(seq[n], None) for n in (5, 12, 36, 79)],
        "subopt_general": [(seq[n], None) for n in (12, 80)],
    }
    reuse = {"edef_general": [(seq[42], tgt[42]), (seq[12], tgt[12]), (seq[5], tgt[5])],
             "subopt_general": [(seq[36], None), (_rand(rng, 12), None), (seq[5], None)]}
    jobs, keys = [], []
    for kind, items in sets.items():
        ss, tt = [s for s, _ in items], [t for _, t in items]
        tt = tt if tt[0] is not None else None
        order = [int(x) for x in rng.permutation(len(ss))]
        for nt in NTS:
            for b in range(len(ss)):                      # workgroup b of the ragged launch, one job each
                jobs.append(("ragged", kind, ss, order[b:b + 1], tt, max(len(s) for s in ss), nt))
                keys.append(("ragged", kind, nt, order[b]))
            for r, (s, t) in enumerate(items):
                jobs.append(("uniform", kind, [s], t, nt))
                keys.append(("uniform", kind, nt, r))
    for kind, items in reuse.items():                     # three lengths, longest first, through ONE slot in one job
        ss, tt = [s for s, _ in items], [t for _, t in items]
        jobs.append(("ragged", kind, ss, [0, 1, 2], tt if tt[0] is not None else None, len(ss[0]), 64))
        keys.append(("reuse", kind, 64, 0))
        for r, (s, t) in enumerate(items):
            jobs.append(("uniform", kind, [s], t, 64))
            keys.append(("reuse_alone", kind, 64, r))
    out = dict(zip(keys, emu_ragged_aux.run_jobs(jobs)))
    return SimpleCases(sets, reuse, out)


class SimpleCases:
    def __init__(self, sets, reuse, out):
        self.sets, self.reuse, self.out = sets, reuse, out


def _bytes(a):
    return np.asarray(a).tobytes()


@pytest.mark.parametrize("kind", ["edef_lds", "edef_general"])
@pytest.mark.parametrize("nt", NTS)
def test_ragged_edef_is_the_uniform_call_per_length(cases, kind, nt):
    items = cases.sets[kind]
    for r, (s, _) in enumerate(items):
        rg, un = cases.out[("ragged", kind, nt, r)], cases.out[("uniform", kind, nt, r)]
        want_bad = "X" in s
        assert int(rg["status"][r]) == int(un["status"][0]) == (ST_BAD_CHAR if want_bad else ST_OK), (len(s), rg["status"], un["status"])
        assert _bytes(rg["edef"][r]) == _bytes(un["edef"][0]), (kind, nt, len(s), rg["edef"][r], un["edef"][0])
        if want_bad:
            assert rg["edef"][r] == 0.0
        else:
            assert 0.0 <= rg["edef"][r] <= 1.0 and np.isfinite(rg["edef"][r])
        # nothing but the sequence's own position was written
        others = [q for q in range(len(items)) if q != r]
        assert all(rg["edef"][q] == -1.0 and rg["status"][q] == -7 for q in others)


@pytest.mark.parametrize("kind", ["subopt_lds", "subopt_general"])
@pytest.mark.parametrize("nt", NTS)
def test_ragged_second_best_is_the_uniform_call_per_length(cases, kind, nt):
    items = cases.sets[kind]
    for r, (s, _) in enumerate(items):
        rg, un = cases.out[("ragged", kind, nt, r)], cases.out[("uniform", kind, nt, r)]
        assert int(rg["status"][r]) == int(un["status"][0]) == ST_OK
        assert int(rg["E2"][r]) == int(un["E2"][0]) and _bytes(rg["E12"][r]) == _bytes(un["E12"][0]), (kind, nt, len(s))
        assert rg["E12"][r, 0] <= rg["E12"][r, 1] and rg["E12"][r, 0] <= 0
        others = [q for q in range(len(items)) if q != r]
        assert all(rg["E2"][q] == -7 and rg["status"][q] == -7 for q in others)


def test_the_two_paths_agree_where_both_fold_a_length(cases):
    """12 nt goes through both second-best kernels: the same two energies (they share kbest_fill)"""
    a = cases.out[("ragged", "subopt_lds", 64, 1)]["E12"][1]
    b = cases.out[("ragged", "subopt_general", 64, 0)]["E12"][0]
    assert _bytes(a) == _bytes(b)


@pytest.mark.parametrize("kind", ["edef_general", "subopt_general"])
def test_a_shorter_successor_in_the_same_slot_sees_nothing_of_its_predecessor(cases, kind):
    got = cases.out[("reuse", kind, 64, 0)]
    for r in range(3):
        alone = cases.out[("reuse_alone", kind, 64, r)]
        assert int(got["status"][r]) == int(alone["status"][0]) == ST_OK
        if kind == "edef_general":
            assert _bytes(got["edef"][r]) == _bytes(alone["edef"][0]), (r, got["edef"][r], alone["edef"][0])
        else:
            assert int(got["E2"][r]) == int(alone["E2"][0]) and _bytes(got["E12"][r]) == _bytes(alone["E12"][0]), r
