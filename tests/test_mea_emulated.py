"""MEA and centroid kernel (desirna_amd/csrc/fold_mea.hpp: mea_kernel, compiled unmodified) in the CPU emulation, workgroups of 64
and 128 threads, against the numpy yardstick of tests/mea_ref.py, which does not prune.  Synthetic matrices whose sums are exact
fix string and value to the bit (the tie rule included); the oracle's pair probabilities of Eterna solutions hold the value to the
derived tolerance.  Energies against oracle.eval_structure."""
import numpy as np
import pytest

from tests import mea_ref as mr
from tests.emu import emu_mea

GAMMAS = (0.25, 1.0, 4.0)
NTS = (64, 128)


@pytest.fixture(scope="module")
def emu(blob):
    return emu_mea.EmuMea(blob)


def synthetic_lengths(lds_max):
    return [1, 4, 5, 63, 64, 65, 130, lds_max - 1, lds_max, lds_max + 1]


@pytest.fixture(scope="module")
def synthetic(emu):
    """{n: (P, {gamma: reference (string, value)}, (centroid, distance))}, computed once"""
    out = {}
    for n in synthetic_lengths(emu.lds_max):
        P = mr.synthetic_matrix(n, seed=1000 + n)
        out[n] = (P, {g: mr.mea(P, g) for g in GAMMAS}, mr.centroid(P))
    return out


def test_lds_bound_is_what_the_header_states(emu):
    assert emu.lds_max == 146 and emu.cand_lds == 4096


@pytest.mark.parametrize("nt", NTS)
def test_synthetic_matrices_to_the_bit(emu, synthetic, nt):
    for n, (P, ref, cen) in synthetic.items():
        for g in GAMMAS:
            forms = [False] + ([True] if n <= emu.lds_max else [])
            res = [emu.run(P, g, nt=nt, lds=f) for f in forms]
            for r in res:
                assert r["E"] is None
                assert (r["mea"][0], r["val"][0]) == ref[g], (n, g, nt)
                assert (r["cen"][0], r["dist"][0]) == cen, (n, g, nt)
                assert r["val"][0] == mr.expected_accuracy(P, r["mea"][0], g)
            if len(res) == 2:                     # LDS and workspace forms: the same bytes
                a, b = res
                assert a["mea"] == b["mea"] and a["cen"] == b["cen"] and a["ncand"][0] == b["ncand"][0]
                assert a["val"].tobytes() == b["val"].tobytes() and a["dist"].tobytes() == b["dist"].tobytes()


def test_pruning_leaves_fewer_candidates_and_the_same_answer(emu, synthetic):
    P, ref, _ = synthetic[130]
    pairs = int((P > 0).sum())
    kept = [int(emu.run(P, g)["ncand"][0]) for g in GAMMAS]
    assert kept[0] < kept[1] < kept[2] <= pairs and kept[0] < pairs, (kept, pairs)    # the reference visits all of them


@pytest.mark.parametrize("nt", NTS)
def test_candidate_lists_beyond_the_lds_pool(emu, nt):
    """a band matrix no pruning thins: more candidates than the LDS lists hold, so they live in the workspace slot, behind M"""
    n, g = 160, 64.0
    P = mr.band_matrix(n, 30, 64)
    ref, cen = mr.mea(P, g), mr.centroid(P)
    for lds in (True, False) if n <= emu.lds_max else (False,):
        r = emu.run(P, g, nt=nt, lds=lds)
        assert r["ncand"][0] == int((P > 0).sum()) > emu.cand_lds
        assert (r["mea"][0], r["val"][0]) == ref and (r["cen"][0], r["dist"][0]) == cen
    n = 140                                       # ... and with M in LDS beside them
    P, g = mr.band_matrix(n, 40, 128), 128.0
    ref = mr.mea(P, g)
    for lds in (True, False):
        r = emu.run(P, g, nt=nt, lds=lds)
        assert r["ncand"][0] == int((P > 0).sum()) > emu.cand_lds
        assert (r["mea"][0], r["val"][0]) == ref


def test_workspace_prefill_does_not_leak(emu, synthetic):
    for n in (5, 65, emu.lds_max + 1):
        P, ref, cen = synthetic[n]
        a = emu.run(P, 1.0, lds=False, fill=0xFF)
        b = emu.run(P, 1.0, lds=False, fill=0x00)
        c = emu.run(P, 1.0, lds=False, fill=0x3F)      # the doubles of the slot read as 0.47...: a stale M would count
        for r in (a, b, c):
            assert (r["mea"][0], r["val"][0]) == ref[1.0] and (r["cen"][0], r["dist"][0]) == cen


@pytest.mark.parametrize("n", [1, 7, 64, 147])
def test_all_zero_matrix(emu, n):
    for nt in NTS:
        for lds in (True, False) if n <= emu.lds_max else (False,):
            r = emu.run(np.zeros((n + 1, n + 1)), 1.0, nt=nt, lds=lds)
            assert r["mea"] == ["." * n] and r["cen"] == ["." * n] and r["val"][0] == float(n) and r["dist"][0] == 0.0
            assert r["ncand"][0] == 0


def test_a_batch_is_its_sequences(emu, synthetic):
    P = np.stack([mr.synthetic_matrix(65, seed=k) for k in range(3)])
    r = emu.run(P, 1.0, nt=128, lds=True)
    for k in range(3):
        one = emu.run(P[k], 1.0, nt=128, lds=True)
        assert r["mea"][k] == one["mea"][0] and r["val"][k] == one["val"][0] and r["dist"][k] == one["dist"][0]


@pytest.fixture(scope="module")
def eterna(oracle, eterna_solutions):
    out = []
    for seq, target in mr.eterna_by_length(eterna_solutions, (12, 36, 80)):
        _, P = oracle.ensemble_defect(seq, target, want_bpp=True)
        out.append((seq, P))
    return out


@pytest.mark.parametrize("nt", NTS)
def test_oracle_matrices(emu, oracle, eterna, nt):
    for seq, P in eterna:
        n = len(seq)
        cen, dist = mr.centroid(P)
        for g in GAMMAS:
            _, want = mr.mea(P, g)
            a = emu.run(P, g, seqs=[seq], nt=nt, lds=True)
            b = emu.run(P, g, seqs=[seq], nt=nt, lds=False)
            assert a["mea"] == b["mea"] and a["val"].tobytes() == b["val"].tobytes() and (a["E"] == b["E"]).all()
            assert a["cen"] == b["cen"] and a["dist"].tobytes() == b["dist"].tobytes()
            db, val = a["mea"][0], a["val"][0]
            print("n = %d gamma = %g: value %.17g, reference %.17g, tol %.3g, candidates %d of %d" %
                  (n, g, val, want, mr.tol(n, g), a["ncand"][0], int((P > 0).sum())))
            assert abs(val - want) <= mr.tol(n, g)
            assert mr.well_formed(P, db) and abs(mr.expected_accuracy(P, db, g) - val) <= mr.tol(n, g)
            assert a["cen"][0] == cen and abs(a["dist"][0] - dist) <= mr.tol(n, g)
            assert a["E"][0, 0] == oracle.eval_structure(seq, db) and a["E"][0, 1] == oracle.eval_structure(seq, cen)


def test_tie_rule(emu):
    """two pairs of one column with the same probability (tests/test_mea_reference.py walks the numbers): "j unpaired" wins a tie
    against a pair, the smaller k a tie between pairs -- whichever lane holds it"""
    P = np.zeros((5, 5))
    P[1, 4] = P[2, 4] = 0.25
    for g, want in ((2.0, ("....", 3.0)), (2.5, ("....", 3.0)), (4.0, ("(..)", 3.75))):
        assert mr.mea(P, g) == want
        for nt in NTS:
            for lds in (True, False):
                r = emu.run(P, g, nt=nt, lds=lds)
                assert (r["mea"][0], r["val"][0]) == want
