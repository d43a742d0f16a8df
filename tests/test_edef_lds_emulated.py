"""The fused inside + outside kernel of short designs (desirna_amd/csrc/fold_edef_lds.hpp: every table in LDS, packed triangle)
compiled unmodified for the CPU.

Two strands: it calls the bodies of cofold_pf_kernel and cofold_outside_kernel, so the defect, every probability and the status
word must be the general pair of kernels' bit for bit (==).  One strand is the instance with an empty second strand, checked
against the oracle's ensemble defect within the project's bound EDEF_TOL = 1e-10, no case left out.

The golden two-strand rows are 17 + 18 nt (heterodimer) and 17 + 17 nt (homodimer); an 18 + 18 pair is drawn at random.  All
emulation jobs of the module run once, side by side in worker processes (the emulation's cost is its barriers)."""
import numpy as np
import pytest

from tests import constructs
from tests.emu import emu_edef_lds
from tests.test_cofold_edef_emulated import EDEF_TOL, defect_from_matrix

ST_BAD_CHAR, ST_TRACEBACK = 1, 2
SENTINEL = -7.0


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _joining_target(la, lb, k):
    """k pairs that join the strands around the nick, dots elsewhere"""
    return "." * (la - k - 1) + "(" * k + "." + "&" + "." + ")" * k + "." * (lb - k - 1)


@pytest.fixture(scope="module")
def emu(blob):
    return emu_edef_lds.EmuEdefLds(blob)


def _two_strand_cases(traj_golden, example_inputs, M):
    rng = np.random.default_rng(41)
    het = [r["sequence"] for r in traj_golden if r["run"] == "RNA_RNA_complex_design_input"]
    hom = [r["sequence"] for r in traj_golden if r["run"] == "Homodimer_design_input"]
    x = _rand(rng, 12, "GGCCAU")
    cases = [("A&U", ".&."), ("G&" + _rand(rng, 7), ".&" + "." * 7), (_rand(rng, 7) + "&C", "." * 7 + "&."),
             (_rand(rng, 18) + "&" + _rand(rng, 18), _joining_target(18, 18, 6)),
             (het[0], example_inputs["RNA_RNA_complex_design_input"]["sec_struct"][0]),
             (het[300], example_inputs["RNA_RNA_complex_design_input"]["sec_struct"][0]),
             (hom[0], example_inputs["Homodimer_design_input"]["sec_struct"][0]),
             (x + "&" + x, "." * 12 + "&" + "." * 12),                                   # homodimer: kappa halved
             (_rand(rng, 13, "GC") + "&" + "A" * 9, "." * 13 + "&" + "." * 9),           # nothing joins
             (_rand(rng, 11, "GGCCAU") + "&" + _rand(rng, 14, "GGCCAU"), _joining_target(11, 14, 4))]
    for cut in (1, M // 2, M - 1):                                                       # the bound exactly
        s = _rand(rng, M, "GGCCAU")
        cases.append((s[:cut] + "&" + s[cut:], "." * cut + "&" + "." * (M - cut)))
    return cases


def _one_strand_cases(M):
    rng = np.random.default_rng(42)
    tg36 = "((((((.((((((((....))))).)).).))))))"
    cases = [("G", "."), ("GAAC", "...."), ("GAAAC", "....."), ("GGGAAACCC", "(((...)))"), (_rand(rng, 36), tg36),
             (_rand(rng, 36, "GGCCAU"), tg36), (_rand(rng, 36), "." * 36), (_rand(rng, 30, "GC"), "((((......))))" + "." * 16)]
    recs = [constructs.hairpin()[27], constructs.interior_record(1, 8), constructs.interior_record(0, 5)] + constructs.multiloop()[:2]
    assert recs[0].name == "hp_30"
    cases += [(r.sequence, r.target) for r in recs]
    s = _rand(rng, M, "GGCCAU")
    cases += [(s, "." * M), (_rand(rng, M), "((((((" + "." * (M - 12) + "))))))")]          # the bound
    assert all(len(s) <= M for s, _ in cases)
    return cases


@pytest.fixture(scope="module")
def results(emu, traj_golden, example_inputs):
    """every emulation job of the module, run once: two strands through the fused and the general kernels at 64 and 128 threads,
    one strand through the fused kernel (every case at 64 threads, the 36-nt ones also at 128)"""
    two = _two_strand_cases(traj_golden, example_inputs, emu.max_two)
    one = _one_strand_cases(emu.max_one)
    jobs, keys = [], []
    for nt in (64, 128):
        for k, (s, t) in enumerate(two):
            jobs += [("lds", s, t, nt, 0.0), ("general", s, t, nt)]
            keys += [("two", "lds", nt, k), ("two", "general", nt, k)]
        for k, (s, t) in enumerate(one):
            if nt == 64 or len(s) == 36:
                jobs.append(("lds", s, t, nt, SENTINEL))
                keys.append(("one", "lds", nt, k))
    return two, one, dict(zip(keys, emu_edef_lds.run_jobs(jobs)))


def test_bounds_cover_the_reference_examples(emu):
    assert emu.max_one >= 36 and emu.max_two >= 36


@pytest.mark.parametrize("nt", [64, 128])
def test_two_strands_bit_identical_to_the_general_kernels(results, nt):
    two, _, res = results
    for k, (s, t) in enumerate(two):
        ed, bpp, F4, st = res[("two", "lds", nt, k)]
        ged, gbpp, gF4, gst = res[("two", "general", nt, k)]
        assert st == gst == 0, s
        assert ed == ged, (s, nt, ed, ged)
        assert (bpp == gbpp).all(), (s, nt)
        assert (F4 == gF4).all(), (s, nt)
        assert abs(ed - defect_from_matrix(bpp, t)) < 1e-12, s
    a = [res[("two", "lds", 64, k)] for k in range(len(two))]
    b = [res[("two", "lds", 128, k)] for k in range(len(two))]
    assert all(x[0] == y[0] and (x[1] == y[1]).all() for x, y in zip(a, b))      # one wave per cell: no workgroup size in the sums


def test_one_strand_against_the_oracle(results, oracle):
    _, one, res = results
    worst_e = worst_p = 0.0
    for (kind, path, nt, k), (ed, bpp, F4, st) in res.items():
        if kind != "one":
            continue
        s, t = one[k]
        oe, ob = oracle.ensemble_defect(s, t, want_bpp=True)
        n = len(s)
        P = np.triu(bpp, 1)
        P[0] = 0.0
        dE, dP = abs(ed - oe), float(np.abs(P - ob).max())
        print("L=%d nt=%d %s |dEdef| %.3e max|dP| %.3e" % (n, nt, t[:20], dE, dP))
        worst_e, worst_p = max(worst_e, dE), max(worst_p, dP)
        assert st == 0, s
        assert dE < EDEF_TOL and dP < EDEF_TOL, (s, t, nt, dE, dP)
        # entries outside 1 <= i < j <= L are the caller's: the sentinel is still there
        keep = np.tril(np.ones((n + 1, n + 1), dtype=bool))
        keep[0] = True
        assert (bpp[keep] == SENTINEL).all() and (bpp[~keep] != SENTINEL).all(), s
    print("one strand: max |dEdef| %.3e max |dP| %.3e over %d runs" % (worst_e, worst_p, sum(k[0] == "one" for k in res)))


def test_one_strand_free_energy_is_the_partition_function(results, oracle):
    """FA of the instance with an empty second strand is the sequence's ensemble free energy (the host reports no F4 for one strand)"""
    _, one, res = results
    for k, (s, t) in enumerate(one):
        if len(s) == 36:
            assert abs(res[("one", "lds", 64, k)][2][0] - oracle.pf(s)) < 1e-9, s


def test_bad_letter_and_batch(emu):
    """the status of the general kernels (ST_BAD_CHAR) and a defect of 0; the rows beside it keep their single-run bits"""
    seqs, tg = ["GGGAAC&GUUCCC", "GGGXAC&GUUCCC", "GCGCAU&AUGCGC"], "((((..&..))))"
    ed, bpp, F4, st = emu.edef(seqs, tg, nt=64, bpp_fill=SENTINEL)
    assert list(st) == [0, ST_BAD_CHAR, 0] and ed[1] == 0.0 and not F4[1].any() and (bpp[1] == SENTINEL).all()
    from tests.emu.emu import cofold_edef
    ged, gbpp, gF4, gst = cofold_edef(seqs, tg, nt=64)
    assert list(gst) == list(st) and (ged == ed).all()
    up = np.triu(np.ones((13, 13), dtype=bool), 1)
    up[0] = False
    for k in (0, 2):
        assert (bpp[k][up] == gbpp[k][up]).all() and (bpp[k][~up] == SENTINEL).all()
    ed1, _, _, st1 = emu.edef(["GGGAAACCC", "GGGANACCC", "GCGAAAGCC"], "(((...)))", nt=64)
    assert list(st1) == [0, ST_BAD_CHAR, 0] and ed1[1] == 0.0 and ed1[0] > 0.0
    assert emu.edef(["GGGAAACCC"], "(((...)))", nt=64)[0][0] == ed1[0]


def test_a_longer_one_leaves_at_once(emu):
    for s in ("A" * (emu.max_one + 1), "A" * emu.max_two + "&A"):
        ed, bpp, F4, st = emu.edef([s], "." * len(s.replace("&", "")), nt=64, bpp_fill=SENTINEL)
        assert list(st) == [ST_TRACEBACK] and ed[0] == 0.0 and (bpp == SENTINEL).all()      # the host never launches it
