"""The GPU's pair probabilities and ensemble defects against a reference that needs no outside recursion
(tests/pair_prob_ref.py: P(i,j) = 1 - exp(-(F[not (i,j)] - F) / kT) from masked inside fills of the oracle; its own noise floor,
measured in tests/test_pair_prob_reference.py, is below 1e-13).  Two strands: cofold_outside_kernel and the two-strand half of
the fused LDS kernel, at every size where the host changes kernels and at cuts of 1 | L-1, up to 150+250.  One strand:
outside_kernel and the fused kernel up to 400 nt, and the ragged entry point.  Bound: EDEF_TOL, for P and for the defect
(largest values seen on an MI355X: |dP| 7.1e-14 at 150+250, |dEdef| 3.6e-15).

Each case runs with the option "edef_lds" 1 and 0 where both kernels exist; the counter "edef_lds_calls" shows which one ran.
Long cases compare a sampled set of entries drawn from the oracle alone (pair_prob_ref.sampled_pairs); the test asserts on the
reference values that the set holds heavy, joining and negligible entries before it looks at the GPU's numbers."""
import numpy as np
import pytest

from tests import pair_prob_ref as R
from tests.probe_params import probe_blob
from tests.test_cofold_edef_emulated import EDEF_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=8, max_L=400, device=0)
    yield e
    e.close()


def _runs(eng, fn, seqs, settings=(1, 0)):
    """[(edef_lds setting, (ed, bpp), fused launches)] of fn(seqs, want_bpp=True) under each setting"""
    out = []
    try:
        for lds in settings:
            eng.set_option("edef_lds", lds)
            c0 = eng.get_option("edef_lds_calls")
            res = fn(seqs, want_bpp=True)
            out.append((lds, res, eng.get_option("edef_lds_calls") - c0))
    finally:
        eng.set_option("edef_lds", 1)
    return out


def _target(oracle, donor, n):
    """the MFE structure of another sequence of the same shape; should that be the open chain, pairs from the ends inwards"""
    tg = R.mfe_structure(oracle, donor).replace("&", "")
    return tg if "(" in tg else R.nested_target(n, R.split(donor)[1], k=max(1, n // 4))


def _check_full(oracle, seqs, target, runs, fits, floor=0.1):
    refs = [R.reference_matrix(oracle, s) for s in seqs]
    wants = [R.reference_defect(oracle, s, target) for s in seqs]
    assert max(P.max() for P in refs) > floor                                  # on the reference alone: something to compare
    for lds, (ed, bpp), calls in runs:
        assert calls == (1 if lds and fits else 0), (lds, calls)
        dP = max(float(np.abs(bpp[k] - refs[k]).max()) for k in range(len(seqs)))
        dE = max(abs(float(ed[k]) - wants[k]) for k in range(len(seqs)))
        print("%s edef_lds=%d: max P_ref %.3f max |dP| %.3e max |dEdef| %.3e" % (seqs[0], lds, max(P.max() for P in refs), dP, dE))
        assert dP < EDEF_TOL and dE < EDEF_TOL, (seqs, lds)


def _check_sampled(oracle, seq, target, seed, per_line, runs):
    pairs = R.sampled_pairs(oracle, seq, seed, per_line)
    p_ref = R.reference_entries(oracle, seq, pairs)
    assert R.sample_is_informative(seq, pairs, p_ref), (seq, seed)
    want = R.reference_defect(oracle, seq, target)
    ii, jj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    for lds, (ed, bpp), calls in runs:
        assert calls == 0, (lds, calls)                                         # beyond the fused kernel's bound
        dP, dE = float(np.abs(bpp[0][ii, jj] - p_ref).max()), abs(float(ed[0]) - want)
        print("%d nt edef_lds=%d: %d entries, max |dP| %.3e |dEdef| %.3e" % (len(R.split(seq)[0]), lds, len(pairs), dP, dE))
        assert dP < EDEF_TOL and dE < EDEF_TOL, (seq, lds)


# ---- two strands

# (label, la, lb as functions of M = cofold_edef_lds_max, alphabet, seed); fits: the fused kernel holds the pair
TWO_FULL = [("2+5", lambda M: (2, 5), "GC", 71), ("18+18", lambda M: (18, 18), "ACGU", 72),
            ("M", lambda M: (M // 2, M - M // 2), "GGCCAU", 73), ("1+(M-1)", lambda M: (1, M - 1), "ACGU", 74),
            ("(M-1)+1", lambda M: (M - 1, 1), "GC", 75), ("M+1", lambda M: (M // 2, M + 1 - M // 2), "GGCCAU", 76)]


def test_two_strands_one_plus_one(eng, oracle):
    """1+1: the only structure beside the open chain is the one pair; its weight exp(-DuplexInit / kT) = 1.3e-3 is the largest
    probability two nucleotides can reach, so that is the floor asserted on the reference here instead of 0.1"""
    seqs = ["G&C", "C&G", "G&U", "A&U", "A&G"]
    eng.set_targets(["()"])
    _check_full(oracle, seqs, "()", _runs(eng, eng.cofold_ensemble_defect, seqs), True, floor=1e-3)


@pytest.mark.parametrize("label,shape,alphabet,seed", TWO_FULL, ids=[c[0] for c in TWO_FULL])
def test_two_strands_full_matrix(eng, oracle, label, shape, alphabet, seed):
    """every allowed pair and the defect against the MFE structure of a third pair: one random pair and one with a planted
    complementary stretch, on the fused kernel and on the general kernels; M + 1 is the first size the fused kernel refuses"""
    M = eng.get_option("cofold_edef_lds_max")
    la, lb = shape(M)
    rng = np.random.default_rng(seed)
    seqs = [R.two_strand_case(rng, la, lb, alphabet, planted) for planted in (False, True)]
    target = _target(oracle, R.two_strand_case(rng, la, lb, alphabet, True), la + lb)
    eng.set_targets([target])
    _check_full(oracle, seqs, target, _runs(eng, eng.cofold_ensemble_defect, seqs), la + lb <= M)


# (label, la, lb, homodimer, planted, seed, pairs drawn per sampled row / column (None = all))
TWO_SAMPLED = [("60+60_homodimer", 60, 60, True, False, 81, None), ("33+90", 33, 90, False, True, 82, None),
               ("100+100", 100, 100, False, False, 83, None), ("150+250", 150, 250, False, True, 84, 3)]


@pytest.mark.parametrize("label,la,lb,homo,planted,seed,per_line", TWO_SAMPLED, ids=[c[0] for c in TWO_SAMPLED])
def test_two_strands_sampled(eng, oracle, label, la, lb, homo, planted, seed, per_line):
    """the general kernels at lengths where a full matrix of masked fills is too many: the MFE pairs, three rows and three
    columns beyond the nick, and the defect against another pair's MFE structure.  150+250, where one masked fill takes 0.2 s:
    3 entries per row / column and the pair's own MFE structure as the target, whose pairs are in the sampled set already, so
    the defect costs one fill per unpaired base only (about 290 fills in all instead of 420)."""
    rng = np.random.default_rng(seed)
    if homo:
        x, y = R.rand_seq(rng, la), R.rand_seq(rng, la)
        seq, donor = x + "&" + x, y + "&" + y[::-1]
    else:
        seq, donor = R.two_strand_case(rng, la, lb, "ACGU", planted), R.two_strand_case(rng, la, lb, "ACGU", True)
    target = _target(oracle, seq if la + lb == 400 else donor, la + lb)
    eng.set_targets([target])
    _check_sampled(oracle, seq, target, seed, per_line, _runs(eng, eng.cofold_ensemble_defect, [seq], settings=(1,)))


# ---- one strand

@pytest.mark.parametrize("over", [0, 1], ids=["edef_lds_max", "edef_lds_max+1"])
def test_one_strand_full_matrix(eng, oracle, over):
    M = eng.get_option("edef_lds_max")
    L = M + over
    rng = np.random.default_rng(91 + over)
    seqs = [R.rand_seq(rng, L, a) for a in R.ALPHABETS]
    target = _target(oracle, R.rand_seq(rng, L, "GGCCAU"), L)
    eng.set_targets([target])
    _check_full(oracle, seqs, target, _runs(eng, eng.ensemble_defect, seqs), L <= M)


ONE_SAMPLED = [(100, 101, None), (200, 102, None), (201, 103, None), (400, 104, 20)]


@pytest.mark.parametrize("L,seed,per_line", ONE_SAMPLED, ids=[str(c[0]) for c in ONE_SAMPLED])
def test_one_strand_sampled(eng, oracle, L, seed, per_line):
    rng = np.random.default_rng(seed)
    seq = R.rand_seq(rng, L, "GGCCAU" if L == 201 else "ACGU")
    target = _target(oracle, R.rand_seq(rng, L), L)
    eng.set_targets([target])
    _check_sampled(oracle, seq, target, seed, per_line, _runs(eng, eng.ensemble_defect, [seq], settings=(1,)))


def test_one_strand_ragged(eng, oracle):
    """one ragged call of 12, edef_lds_max, edef_lds_max + 1 and 100 nt, each against a target of its own: the defect from masked
    fills.  With edef_lds on the two short ones share one fused launch."""
    M = eng.get_option("edef_lds_max")
    rng = np.random.default_rng(111)
    lens = (12, M, M + 1, 100)
    seqs = [R.rand_seq(rng, n, R.ALPHABETS[k % 3]) for k, n in enumerate(lens)]
    targets = ["((((....))))"] + [_target(oracle, R.rand_seq(rng, n), n) for n in lens[1:]]
    assert len(set(targets)) == 4 and all("(" in t for t in targets)
    wants = np.array([R.reference_defect(oracle, s, t) for s, t in zip(seqs, targets)])
    eng.set_targets_ragged(targets)
    try:
        for lds in (1, 0):
            eng.set_option("edef_lds", lds)
            c0 = eng.get_option("edef_lds_calls")
            ed = eng.ensemble_defect_ragged(seqs, [0, 1, 2, 3])
            assert eng.get_option("edef_lds_calls") - c0 == lds
            d = np.abs(ed - wants)
            print("ragged edef_lds=%d: |dEdef| %s" % (lds, " ".join("%.3e" % x for x in d)))
            assert d.max() < EDEF_TOL, (lds, d)
    finally:
        eng.set_option("edef_lds", 1)


# ---- another parameter set

def test_distinct_probe_parameters():
    """engine and oracle on the "distinct" probe blob (tests/probe_params.py: no two tables equal, MLbase != 0): one 20+25 pair and
    strands of edef_lds_max and of 60 nt, every allowed pair, both settings"""
    from desirna_amd import engine
    from oracle.pyoracle import Oracle
    blob = probe_blob("distinct")
    orc = Oracle(blob)
    rng = np.random.default_rng(121)
    e = engine.Engine(max_R=4, max_L=60, device=0, params=blob)
    try:
        M = e.get_option("edef_lds_max")
        pair, donor = (R.two_strand_case(rng, 20, 25, "ACGU", True) for _ in range(2))
        target = _target(orc, donor, 45)
        e.set_targets([target])
        _check_full(orc, [pair], target, _runs(e, e.cofold_ensemble_defect, [pair]), True)
        for L in (M, 60):
            seq = R.rand_seq(rng, L)
            target = _target(orc, R.rand_seq(rng, L), L)
            e.set_targets([target])
            _check_full(orc, [seq], target, _runs(e, e.ensemble_defect, [seq]), L <= M)
    finally:
        e.close()
