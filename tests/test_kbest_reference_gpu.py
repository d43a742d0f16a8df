"""The ranked-structure calls of the engine against an exact reference for EVERY rank, one and two strands:
drna_subopt_structs_batch, drna_cofold_subopt_structs_batch, drna_cofold_subopt_energy_batch.

The references are the oracle's serial K-list fill (any length) and, on the sparse long cases, exhaustive enumeration; both are
held to each other on the CPU by tests/test_kbest_reference.py.  Every answer goes through the one rule kbest_ref.check_ranked:
energies equal rank for rank, strings balanced, distinct and worth their energy, and -- where enumeration ran -- no structure
below the last returned energy missing."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import kbest_ref as KR
from tests.probe_params import probe_blob

pytestmark = pytest.mark.gpu

INF_REF = KR.INF_REF
KS = (3, 4, 5, 8)                 # both kernel instances (lists of 4 and of 8) and a cut of each list


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=128, max_L=400, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def probe():
    """(engine, oracle) under the `distinct` probe parameter set"""
    from desirna_amd import engine
    from oracle import pyoracle
    blob = probe_blob("distinct")
    e = engine.Engine(max_R=16, max_L=100, device=0, params=blob)
    yield e, pyoracle.Oracle(blob)
    e.close()


def _fill8(oracle, seqs):
    """oracle.kbest_energies(s, 8) of every sequence (the oracle calls release the GIL)"""
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda s: oracle.kbest_energies(s, 8), seqs))


def _enum8(oracle, seqs):
    def one(s):
        c = oracle.count_structures(s)
        assert c <= KR.CAP, (s, c)
        E, ss, cnt = oracle.enum_kbest(s, 8)
        assert cnt == c, s
        return E, ss
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, seqs))


def _ranked(eng, seqs, K):
    return eng.cofold_subopt_structs(seqs, K) if "&" in seqs[0] else eng.subopt_structs(seqs, K)


def _check_batch(eng, oracle, seqs, ref, enumerated=False):
    """one call per K; ref[k] = the 8 reference energies (fill), or (energies, strings) of the enumeration"""
    for K in KS:
        E, ss = _ranked(eng, seqs, K)
        for k, s in enumerate(seqs):
            if enumerated:
                KR.check_ranked(oracle, s, E[k], ss[k], ref[k][0], ref[k][1])
            else:
                KR.check_ranked(oracle, s, E[k], ss[k], ref[k])


def _by_shape(seqs):
    groups = {}
    for s in seqs:
        groups.setdefault((s.find("&"), len(s)), []).append(s)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------- ranked structures

@pytest.mark.parametrize("L", KR.GPU_LENGTHS)
def test_one_strand_every_rank(eng, oracle, L):
    seqs = KR.gpu_one_strand(L)
    _check_batch(eng, oracle, seqs, _fill8(oracle, seqs))


def test_named_cases_against_enumeration(eng, oracle):
    """the sequences and pairs of kbest_ref.NAMED_ONE / NAMED_TWO, on which a mistake in the list handling changes a rank"""
    for s in list(KR.NAMED_ONE.values()) + list(KR.NAMED_TWO.values()):
        _check_batch(eng, oracle, [s], _enum8(oracle, [s]), enumerated=True)


def test_one_strand_sparse_against_enumeration(eng, oracle):
    """100 - 260 nt with hairpins beyond 30, interior loops at MAXLOOP, three-stem multiloops that span more than one wave"""
    for seqs in _by_shape(list(KR.sparse_one_strand().values())):
        assert len(seqs[0]) >= 100
        _check_batch(eng, oracle, seqs, _enum8(oracle, seqs), enumerated=True)


@pytest.mark.parametrize("la,lb", KR.GPU_PAIR_SHAPES + ((30, 30),))
def test_two_strands_every_rank(eng, oracle, la, lb):
    seqs = KR.gpu_two_strands(la, lb) + ([KR.gpu_homodimer(30)] if (la, lb) == (30, 30) else [])
    _check_batch(eng, oracle, seqs, _fill8(oracle, seqs))


def test_two_strands_sparse_against_enumeration(eng, oracle):
    for seqs in _by_shape(list(KR.sparse_two_strands().values())):
        _check_batch(eng, oracle, seqs, _enum8(oracle, seqs), enumerated=True)


# ---------------------------------------------------------------------------------------------- second-best co-fold energies

def _e2(e12):
    return e12[1] if e12[1] < INF_REF and e12[1] - e12[0] <= 4900 else 0


def test_cofold_second_best_energies(eng, oracle):
    """drna_cofold_subopt_energy_batch against the oracle fill (K = 2) on both sides of the LDS / general path switch, with the
    nick at 1, in the middle and at L - 1, and at 64+64 and 100+100"""
    M = eng.get_option("subopt_lds_max")
    assert 8 <= M < 128
    shapes = [(cut, L - cut) for L in (M, M + 1) for cut in (1, L // 2, L - 1)] + [(64, 64), (100, 100)]
    rng = np.random.default_rng([KR.SEED, 11])
    for la, lb in shapes:
        seqs = [KR._rand(rng, la) + "&" + KR._rand(rng, lb), KR._rand(rng, la, "GGCCAU") + "&" + KR._rand(rng, lb, "GGCCAU"),
                KR._rand(rng, la, "GC") + "&" + KR._rand(rng, lb, "GC"), "A" * la + "&" + "A" * lb]
        with ThreadPoolExecutor(8) as ex:
            want = list(ex.map(lambda s: oracle.kbest_energies(s, 2), seqs))
        E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
        for k, s in enumerate(seqs):
            assert [int(E12[k, 0]), int(E12[k, 1])] == want[k], (s, E12[k], want[k])
            assert int(E2[k]) == _e2(want[k]), s
        assert [int(x) for x in eng.cofold_subopt_energy(seqs)] == [_e2(w) for w in want], (la, lb)


# ---------------------------------------------------------------------------------------------- probe parameters, batching

def test_probe_parameters(probe):
    e, O = probe
    rng = np.random.default_rng([KR.SEED, 12])
    one = [KR._rand(rng, 36) for _ in range(3)] + [KR._rand(rng, 36, "GC"), KR._rand(rng, 36, "GGCCAU")]
    two = [KR._rand(rng, 18, a) + "&" + KR._rand(rng, 18, a) for a in ("ACGU", "ACGU", "ACGU", "GC", "GGCCAU")]
    for seqs in (one, two):
        E, ss = _ranked(e, seqs, 8)
        for k, (s, ref) in enumerate(zip(seqs, _fill8(O, seqs))):
            KR.check_ranked(O, s, E[k], ss[k], ref)
    for seqs in ([s for s in KR.sparse_one_strand().values() if len(s) == 100],
                 [s for s in KR.sparse_two_strands().values() if s.index("&") == 50 and len(s) == 101]):
        assert len(seqs) >= 3
        E, ss = _ranked(e, seqs, 8)
        for k, (s, (rE, rss)) in enumerate(zip(seqs, _enum8(O, seqs))):
            KR.check_ranked(O, s, E[k], ss[k], rE, rss)


def test_batches_beyond_one_workspace_chunk(eng, oracle):
    """40 sequences / 20 pairs in one call (a K-best workspace chunk holds 16): EVERY row against the reference"""
    rng = np.random.default_rng([KR.SEED, 13])
    one = [KR._rand(rng, 36, ("ACGU", "GGCCAU")[k % 2]) for k in range(40)]
    two = [KR._rand(rng, 18) + "&" + KR._rand(rng, 18) for _ in range(20)]
    for seqs in (one, two):
        ref = _fill8(oracle, seqs)
        for K in (4, 8):
            E, ss = _ranked(eng, seqs, K)
            for k, s in enumerate(seqs):
                KR.check_ranked(oracle, s, E[k], ss[k], ref[k])
