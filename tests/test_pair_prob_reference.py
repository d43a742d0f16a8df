"""Pair probabilities from forbidden-pair free energies (tests/pair_prob_ref.py): a reference for the outside recursions that
needs no outside recursion, at sizes no enumeration reaches.

  a. the masked inside fills (orc_pf_forbid, orc_cofold_pf_forbid) are what they claim: against enumeration, and fi == 0 is
     bit-equal to the unmasked fill;
  b. the oracle's outside recursion (orc_ensemble_defect) against the reference at 40 to 400 nt: this measures the reference's
     own noise floor;
  c. the two-strand outside kernels (fold_cofold_outside.hpp, emulated on the CPU) against the reference up to 30+30.
The GPU builds are compared with the same reference in tests/test_pair_prob_reference_gpu.py."""
import numpy as np
import pytest

from tests import pair_prob_ref as R
from tests.emu.emu import Emu, cofold_edef_many
from tests.probe_params import probe_blob
from tests.test_cofold_edef_emulated import EDEF_TOL, KT, homodimer_cases
from tests.test_cofold_subopt_emulated import _enumeration_cases, cofold_structures
from tests.test_oracle_golden import _enumerate

# orc_ensemble_defect against the reference is the reference's own noise floor (b); EDEF_TOL has to stay 100 times above it
NOISE_BOUND = EDEF_TOL / 100


def _masked_free_energies(structs, w, pairs, n):
    """-kT log of the weight of the structures without the pair, per pair, and of those that leave i unpaired, per base: sums
    over the structures that remain, never Z minus something"""
    has = np.zeros((len(structs), len(pairs)), dtype=bool)
    paired = np.zeros((len(structs), n + 1), dtype=bool)
    col = {p: k for k, p in enumerate(pairs)}
    for s, db in enumerate(structs):
        for p in R.pairs_of(db):
            has[s, col[p]] = True
            paired[s, p[0]] = paired[s, p[1]] = True
    Fp = np.array([-KT * np.log(w[~has[:, k]].sum()) for k in range(len(pairs))])
    Fb = np.array([-KT * np.log(w[~paired[:, i]].sum()) for i in range(1, n + 1)])
    return Fp, Fb


def test_masked_fill_one_strand_against_enumeration(oracle):
    """every structure of a sequence of at most 16 nt, weighted by orc_boltzmann_weight (a structure walk that shares nothing
    with the fill): F[not (i,j)] and F[not i] to 1e-11 kcal/mol, the bound test_oracle_golden.py holds the unmasked F to"""
    rng = np.random.default_rng(41)
    seqs = ["GGGAAACGGAAACCGA", "GGACGAAAGCAAAACC", "GCAAGCAAAGCAAAGC"]
    seqs += [R.rand_seq(rng, int(rng.integers(9, 17)), R.ALPHABETS[k % 3]) for k in range(9)]
    worst, seen = 0.0, 0
    for seq in seqs:
        n = len(seq)
        structs = _enumerate(seq, oracle)
        w = np.array([oracle.boltzmann_weight(seq, db) for db in structs])
        pairs = R.allowed_pairs(seq)
        assert {p for db in structs for p in R.pairs_of(db)} <= set(pairs)
        Fp, Fb = _masked_free_energies(structs, w, pairs, n)
        got_p = oracle.pf_forbid(seq, [p[0] for p in pairs], [p[1] for p in pairs]) if pairs else np.zeros(0)
        got_b = oracle.pf_forbid(seq, list(range(1, n + 1)), 0)
        d = max(float(np.abs(got_p - Fp).max()) if pairs else 0.0, float(np.abs(got_b - Fb).max()))
        worst, seen = max(worst, d), seen + len(pairs)
        assert d < 1e-11, seq
        for (i, j), f in list(zip(pairs, got_p))[:3]:                       # the scalar entry, either order of the two indices
            assert oracle.pf_forbid(seq, i, j) == f == oracle.pf_forbid(seq, j, i)
    print("one strand: %d pairs, max |dF| %.3e kcal/mol" % (seen, worst))
    assert seen > 200


@pytest.mark.parametrize("kind", ["hetero", "homo"])
@pytest.mark.parametrize("name", ["turner1999", "distinct_sharp"])
def test_masked_fill_two_strands_against_enumeration(name, kind):
    """enumerate_ensemble's rule (weight exp(-E / kT) of the oracle's two-strand evaluation, connected structures halved for
    equal strands) over the structures that lack the pair / leave i unpaired.

    "distinct_sharp" (tests/probe_params.py): the integer evaluation and the partition function's loop model give every structure
    the same energy, so every case enters and F[not (i,j)], F[not i] agree to 1e-9 kcal/mol, rounding only: the bound
    test_probe_params_oracle.py::test_cofold_against_enumeration holds the unmasked FAB to.

    "turner1999": a case enters under the condition of test_probabilities_against_enumeration (the two loop models agree on F
    to 1e-6 kcal/mol), with its caps on how many may drop out.  Agreement on F does not carry over to a sub-ensemble: forbid the
    dominant pair and structures whose dangle-like terms lie where smooth() is curved take over (CCCGG&GGGC: |dF[not (2,9)]| =
    2e-5).  What the condition does bound is the weight ratio Z[not ...] / Z = 1 - P, the quantity that test holds to 1e-5, so
    the masked fills are held to the same: |exp(-(F[not ...] - F) / kT) - Z_enum[not ...] / Z_enum| < 1e-5."""
    from oracle.pyoracle import Oracle
    oracle = Oracle(probe_blob(name))
    sharp = name == "distinct_sharp"
    cases, need = (_enumeration_cases(), 40) if kind == "hetero" else (homodimer_cases(), 9)
    if sharp:
        need = len(cases)
    entered, worst = 0, 0.0
    for s in cases:
        a, b = s.split("&")
        flat, cut = a + b, len(a)
        n = len(flat)
        structs = cofold_structures(flat, cut)
        w = np.array([np.exp(-oracle.eval_structure(flat, db, cut) / 100.0 / KT) for db in structs])
        if a == b:
            w *= np.array([0.5 if any(i <= cut < j for i, j in R.pairs_of(db)) else 1.0 for db in structs])
        F, F_enum = oracle.cofold_pf(s)[3], -KT * np.log(w.sum())
        if abs(F_enum - F) >= (1e-9 if sharp else 1e-6):
            continue
        entered += 1
        pairs = R.allowed_pairs(s)
        assert {p for db in structs for p in R.pairs_of(db)} <= set(pairs)
        Fp, Fb = _masked_free_energies(structs, w, pairs, n)
        got_p = oracle.cofold_pf_forbid(s, [p[0] for p in pairs], [p[1] for p in pairs])[:, 3] if pairs else np.zeros(0)
        got_b = oracle.cofold_pf_forbid(s, list(range(1, n + 1)), 0)[:, 3]
        got, want = np.concatenate([got_p, got_b]), np.concatenate([Fp, Fb])
        if sharp:
            d = float(np.abs(got - want).max())
            assert d < 1e-9, s
        else:
            d = float(np.abs(np.exp(-(got - F) / KT) - np.exp(-(want - F_enum) / KT)).max())
            assert d < 1e-5, s
        worst = max(worst, d)
    print("%s %s: %d cases entered, max deviation %.3e" % (name, kind, entered, worst))
    assert entered >= need, entered


def test_no_mask_is_the_unmasked_fill(oracle):
    """fi == 0: the bits of orc_pf / orc_cofold_pf, through the scalar and the batched entry; the batch equals the scalar calls"""
    rng = np.random.default_rng(42)
    for k, L in enumerate((5, 16, 37, 120, 200)):
        s = R.rand_seq(rng, L, R.ALPHABETS[k % 3])
        assert oracle.pf_forbid(s, 0, 0) == oracle.pf(s) == oracle.pf_forbid(s, [0, 0], [0, 7])[0]
        pairs = R.allowed_pairs(s)[:5]
        batch = oracle.pf_forbid(s, [p[0] for p in pairs] + [3], [p[1] for p in pairs] + [0])
        assert list(batch) == [oracle.pf_forbid(s, i, j) for i, j in pairs] + [oracle.pf_forbid(s, 3)]
        for c in (s[:L // 3] + "&" + s[L // 3:], s[:L // 2] + "&" + s[:L // 2], s[:1] + "&" + s[1:]):
            assert oracle.cofold_pf_forbid(c, 0, 0) == oracle.cofold_pf(c) == tuple(oracle.cofold_pf_forbid(c, [0], [0])[0])
            pairs = R.allowed_pairs(c)[:5]
            batch = oracle.cofold_pf_forbid(c, [p[0] for p in pairs] + [2], [p[1] for p in pairs] + [0])
            assert [tuple(r) for r in batch] == [oracle.cofold_pf_forbid(c, i, j) for i, j in pairs] + [oracle.cofold_pf_forbid(c, 2)]


def test_mask_of_a_base_is_the_mask_of_all_its_pairs(oracle):
    """F[not i] leaves the monomer of the other strand alone, and a base that pairs with nothing changes nothing"""
    s = "GGGCAUCC&GGAUGCAC"
    F = oracle.cofold_pf(s)
    Fi = oracle.cofold_pf_forbid(s, 3)
    assert Fi[1] == F[1] and Fi[0] > F[0] and Fi[3] > F[3]
    assert oracle.cofold_pf_forbid("GGGCACCC&AAAAAAAA", 12) == oracle.cofold_pf("GGGCACCC&AAAAAAAA")
    assert oracle.pf_forbid("GGGAAAACCC", 5, 6) == oracle.pf("GGGAAAACCC")          # not a pair of the model: nothing to forbid


# ---- b. the oracle's outside recursion against the reference

ONE_STRAND = ((40, None, 51), (100, None, 52), (200, "sample", 53), (400, "sample", 54))


@pytest.mark.parametrize("L,mode,seed", ONE_STRAND)
def test_oracle_outside_against_reference(oracle, L, mode, seed):
    """orc_ensemble_defect's matrix and defect against the reference: every allowed pair at 40 and 100 nt, the sampled set at
    200 and 400 nt, the defect against the MFE structure of another sequence (one fill per unpaired base and per target pair).
    Two recursions that share only the inside fill: their distance is the reference's noise floor.  Largest values seen:
    max |dP| 8.0e-15 (40 nt), 4.3e-14 (100 nt), 2.2e-14 (200 nt), 7.8e-14 (400 nt); |dEdef| 5.1e-15 at most.  Asserted below
    EDEF_TOL / 100 = 1e-12."""
    rng = np.random.default_rng(seed)
    for alphabet in (R.ALPHABETS if L <= 100 else R.ALPHABETS[:1]):
        s, other = R.rand_seq(rng, L, alphabet), R.rand_seq(rng, L, alphabet)
        target = oracle.mfe(other)[0]
        assert "(" in target
        ed, bpp = oracle.ensemble_defect(s, target, want_bpp=True)
        pairs = R.allowed_pairs(s) if mode is None else R.sampled_pairs(oracle, s, seed, per_line=20 if L == 400 else None)
        p_ref = R.reference_entries(oracle, s, pairs)
        if mode is not None:
            assert R.sample_is_informative(s, pairs, p_ref)
        else:
            assert p_ref.max() > 0.1
        dP = float(np.abs(np.array([bpp[i, j] for i, j in pairs]) - p_ref).max())
        dE = abs(ed - R.reference_defect(oracle, s, target))
        print("L=%d %s: %d pairs, max |dP| %.3e |dEdef| %.3e" % (L, alphabet, len(pairs), dP, dE))
        assert dP < NOISE_BOUND and dE < NOISE_BOUND, (L, alphabet)


def test_row_sums_of_the_reference(oracle):
    """the two formulas agree with each other: sum_j P(i,j) from F[not i] against the sum of the entries from F[not (i,j)]"""
    rng = np.random.default_rng(55)
    for s in (R.rand_seq(rng, 60), R.two_strand_case(rng, 21, 30, "ACGU", True)):
        n = len(R.split(s)[0])
        P = R.reference_matrix(oracle, s)
        rows = oracle.pair_probs_by_forbidding(s, bases=range(1, n + 1))[1]
        assert np.abs((P + P.T)[1:, 1:].sum(1) - rows).max() < NOISE_BOUND, s
        assert rows.max() > 0.5


# ---- c. the emulated two-strand kernels against the reference

def _two_strand_cases():
    """18+18 twice (the neighbour lends the target), 25+32 twice, 1+30, 30+1 and a homodimer 30+30, alternately random and with
    a planted complementary stretch"""
    rng = np.random.default_rng(61)
    out = []
    for la, lb, k in ((18, 18, 2), (25, 32, 2), (1, 30, 2), (30, 1, 2)):
        for _ in range(k):
            out.append(R.two_strand_case(rng, la, lb, R.ALPHABETS[len(out) % 3], planted=len(out) % 2 == 1))
    x = R.rand_seq(rng, 30, "ACGU")
    return out + [x + "&" + x]


def _target_from_neighbour(oracle, cases, k):
    """the MFE structure of another sequence of the batch with the same strand lengths (the homodimer: of the 25+32 case's
    letters cut to 30+30, a structure that is not symmetric)"""
    cut = cases[k].index("&")
    for other in cases[k + 1:] + cases[:k]:
        if other.index("&") == cut and len(other) == len(cases[k]):
            return oracle.cofold_mfe(other)[0]
    flat = cases[2].replace("&", "") + cases[3].replace("&", "")
    return oracle.cofold_mfe(flat[:cut] + "&" + flat[cut:len(cases[k]) - 1])[0]


def test_emulated_cofold_outside_against_reference(oracle):
    """cofold_pf_kernel + cofold_outside_kernel (emulated) against the reference, every allowed pair and the defect for the MFE
    structure of the neighbouring case: 18+18, 25+32, 1+30, 30+1 (random and with a planted complementary stretch) and a
    homodimer 30+30.  Bound EDEF_TOL; largest values seen: max |dP| 1.0e-14, |dEdef| 7.8e-16."""
    cases = _two_strand_cases()
    targets = [_target_from_neighbour(oracle, cases, k) for k in range(len(cases))]
    got = cofold_edef_many(cases, targets, nt=64)
    heavy = 0
    for s, tg, (ed, bpp, F4, st) in zip(cases, targets, got):
        assert st == 0, s
        P = R.reference_matrix(oracle, s)
        cut = s.index("&")
        heavy += P[1:cut + 1, cut + 1:].max() > 0.1
        dP, dE = float(np.abs(bpp - P).max()), abs(ed - R.reference_defect(oracle, s, tg))
        print("%s %s: max P_ref %.3f (joining %.3f) max |dP| %.3e |dEdef| %.3e" % (s, tg, P.max(), P[1:cut + 1, cut + 1:].max(), dP, dE))
        assert dP < EDEF_TOL, s
        assert dE < EDEF_TOL, (s, tg)
    assert heavy >= 3                                  # pairs that join the strands carry weight in at least three of the cases


def test_emulated_cofold_outside_under_the_distinct_probe():
    """the same under the "distinct" probe parameter set (no two tables equal, MLbase != 0), oracle and kernel on one blob"""
    from oracle.pyoracle import Oracle
    blob = probe_blob("distinct")
    orc = Oracle(blob)
    rng = np.random.default_rng(62)
    seqs = [R.two_strand_case(rng, 20, 25, "ACGU", True) for _ in range(2)]
    tg = orc.cofold_mfe(seqs[1])[0]
    ed, bpp, F4, st = Emu(blob).cofold_edef(seqs[:1], tg)
    assert st[0] == 0
    P = R.reference_matrix(orc, seqs[0])
    assert P.max() > 0.1
    dP, dE = float(np.abs(bpp[0] - P).max()), abs(ed[0] - R.reference_defect(orc, seqs[0], tg))
    print("distinct probe %s: max |dP| %.3e |dEdef| %.3e" % (seqs[0], dP, dE))
    assert dP < EDEF_TOL and dE < EDEF_TOL
