"""Accessible regions on the GPU (Engine.unpaired_free_energy: pf_kernel<1024, true>, and access_lds_kernel<1024> up to the host's
bound): the masked free energies against enumeration (tests/access_ref.py) and the pinned masked fill oracle.pf_forbid within
1e-9 kcal/mol, the chunking, the routing between the two kernels, the all-zero mask against the score batch, and one seeded
design with an >accessible region."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import access_ref as ar, pair_prob_ref

pytestmark = pytest.mark.gpu

TOL = 1e-9                                            # EPF_TOL_ORACLE
TARGET36 = "((((((.((((((((....))))).)).).))))))"


def _rand(n, tag, alphabet="ACGU"):
    return pair_prob_ref.rand_seq(np.random.default_rng([ar.SEED, 4, tag, n]), n, alphabet)


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=16, max_L=260, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lds_max(eng):
    return eng.get_option("access_lds_max")


def _in_calls(eng, seqs, masks, per_call=9):
    """F (R, M) from calls of at most `per_call` masks each (R = len(seqs) <= 3)"""
    assert len(seqs) <= 3
    return np.concatenate([eng.unpaired_free_energy(seqs, masks[k:k + per_call]) for k in range(0, masks.shape[0], per_call)], axis=1)


# 36 nt within the enumeration's cap: seeded draws over A-rich alphabets (AAACGU, AAGGCC, AACGGU), kept when the REFERENCE counted
# 5e3 - 1e5 structures and a window of 4 that costs more than 1 kcal/mol to free (a random ACGU sequence of 36 nt has ~1e7)
# 14 nt: two of access_ref.DENSE_REFERENCE and one more ACGU draw kept by the same rule (a mask that costs more than 0.5 kcal/mol)
DENSE = {14: ("GCGGAAGAACUCUU", "CCCCGCGCGCGGCG", "AAAGUGUCGCGACG"),
         36: ("AAAGAACUAGCAGCCAAGACAUGAAGCACGGAAAGA", "AGAGAGGACAGACCCAGGGCAGAGGACAACAAGAGA",
                        "AGGAAAGAAGAAUGCAAGAUAGUCGGGAGGAGCGAA")}


@pytest.mark.parametrize("n", (14, 36))
def test_dense_against_enumeration(eng, oracle, n):
    """three dense sequences per length, R = 3 and at most 9 masks per call"""
    seqs = list(DENSE[n])
    rng = np.random.default_rng([ar.SEED, 5, n])
    picks = np.concatenate([ar.single_masks(n)[rng.choice(n, 6, replace=False)], ar.window_masks(n, 4, every=max(1, n // 6)),
                            ar.random_masks(n, 6, 3)])
    ref = np.array([ar.check_case(ar.Ensemble(oracle, s), picks) for s in seqs])
    for lds in (1, 0):
        eng.set_option("access_lds", lds)
        F = _in_calls(eng, seqs, picks)
        assert F.shape == ref.shape and np.abs(F - ref).max() <= TOL, (lds, np.abs(F - ref).max())
    eng.set_option("access_lds", 1)


def test_single_positions_against_the_masked_fill(eng, oracle, lds_max):
    """both sides of the host's bound and of the kernel's, as the host routes them (access_lds = 1) and with the LDS kernel at every
    length it holds (2: beyond the kernel's bound the general kernel again)"""
    kernel_max = eng.get_option("access_lds_kernel_max")
    assert lds_max <= kernel_max
    lengths = sorted({lds_max, lds_max + 1, 64, 65, kernel_max, kernel_max + 1, 129, 200, 260})
    for n in lengths:
        seqs = [_rand(n, 10 + k) for k in range(3)]
        pos = ar.inner_positions(n, 1)
        ref = np.array([oracle.pf_forbid(s, pos, 0) for s in seqs])
        assert (ref - np.array([[oracle.pf(s)] for s in seqs])).max() > ar.MIN_EOPEN
        for mode in (1, 2) if n <= kernel_max else (1,):
            eng.set_option("access_lds", mode)
            c0 = eng.get_option("access_lds_calls")
            F = _in_calls(eng, seqs, ar.mask_rows(n, [[p] for p in pos]))
            assert (eng.get_option("access_lds_calls") > c0) == (n <= (lds_max if mode == 1 else kernel_max))
            assert np.abs(F - ref).max() <= TOL, (n, mode, np.abs(F - ref).max())
    eng.set_option("access_lds", 1)


@pytest.mark.parametrize("name", ("seeded_100_12", "seeded_200_14"))
def test_sparse_windows_against_enumeration(eng, oracle, name):
    seq = ar.sparse_cases()[name]
    masks = ar.window_masks(len(seq), 8, every=8)
    ref = ar.check_case(ar.Ensemble(oracle, seq), masks)
    F = _in_calls(eng, [seq], masks)
    assert np.abs(F[0] - ref).max() <= TOL, np.abs(F[0] - ref).max()


def test_chunking_is_invisible():
    """R M = 15 folds through two workspace slots and through sixteen: the same bits, on either kernel (access_lds = 2: the LDS
    kernel beyond the host's bound)"""
    from desirna_amd import engine
    seqs = [_rand(70, 20 + k) for k in range(3)]
    masks = np.concatenate([np.zeros((1, 70), np.uint8), ar.window_masks(70, 8, every=17)])[:5]
    assert len(seqs) * masks.shape[0] == 15
    got = {}
    for max_R in (2, 16):
        for lds in (2, 0):
            e = engine.Engine(max_R=max_R, max_L=70, device=0)
            e.set_option("access_lds", lds)
            got[(max_R, lds)] = e.unpaired_free_energy(seqs, masks)
            assert (e.get_option("access_lds_calls") > 0) == (lds == 2)
            e.close()
    for lds in (2, 0):
        assert got[(2, lds)].tobytes() == got[(16, lds)].tobytes()
    assert np.abs(got[(16, 2)] - got[(16, 0)]).max() <= TOL


def test_routing(eng, lds_max):
    calls = lambda: eng.get_option("access_lds_calls")
    short, long_ = [_rand(lds_max, 30 + k) for k in range(2)], [_rand(lds_max + 1, 30 + k) for k in range(2)]
    m_short, m_long = ar.window_masks(lds_max, 8, every=20), ar.window_masks(lds_max + 1, 8, every=20)
    assert eng.get_option("access_lds") == 1
    c0 = calls()
    F1 = eng.unpaired_free_energy(short, m_short)
    assert calls() == c0 + 1                                   # within the bound: the LDS kernel, one launch
    eng.unpaired_free_energy(long_, m_long)
    assert calls() == c0 + 1                                   # beyond it: the general kernel
    eng.set_option("access_lds", 0)
    F0 = eng.unpaired_free_energy(short, m_short)
    assert calls() == c0 + 1
    eng.set_option("access_lds", 1)
    assert np.abs(F1 - F0).max() <= TOL
    assert eng.last_access_timing() > 0.0


def test_zero_mask_is_the_score_batch_epf(eng, lds_max):
    from desirna_amd import engine
    for n in (36, lds_max + 1, 200):
        seqs = [_rand(n, 40 + k) for k in range(3)]
        Epf = eng.score_batch(seqs, engine.NEED_PF)["Epf"]
        F = eng.unpaired_free_energy(seqs, np.zeros((1, n), np.uint8))
        assert np.abs(F[:, 0] - Epf).max() <= TOL
        Eopen, p = eng.opening_energy(seqs, ar.window_masks(n, 8, every=n // 3))
        Eopen2, p2 = eng.opening_energy(seqs, ar.window_masks(n, 8, every=n // 3), Epf=Epf)
        assert np.abs(Eopen - Eopen2).max() <= 2 * TOL and (Eopen > -TOL).all() and (p <= 1 + 1e-9).all()
        assert np.allclose(p, np.exp(-Eopen / engine.KT), rtol=0, atol=1e-12)


def test_bad_input(eng):
    from desirna_amd import engine
    with pytest.raises(engine.EngineError) as ex:
        eng.unpaired_free_energy(["GGGAAACCC", "GGGAXACCC"], "..xxx....")
    assert ex.value.code == -4 and "sequence 1" in str(ex.value)
    with pytest.raises(ValueError):
        eng.unpaired_free_energy(["GGGAAACCC"], "..xx")
    with pytest.raises(ValueError):
        eng.unpaired_free_energy(["GGGAAACCC"], "..xxy....")
    with pytest.raises(engine.EngineError):
        eng.unpaired_free_energy(["A" * 261], np.zeros((1, 261), np.uint8))


def test_design_with_a_region(oracle):
    """one seeded run_design_fast, 2 steps x 5 iterations x 4 replicas on a 36-nt target with a region: every record's opening
    energy recomputed with oracle.pf and the reference, and its scoring function the stated sum.  The region is ONE position of
    the hairpin loop, so that the pinned masked fill oracle.pf_forbid(seq, i, 0) is the exact reference for whatever sequence the
    run visits (a designed 36-nt sequence has too many structures to enumerate)."""
    from desirna_amd import design, engine
    from desirna_amd import energy_scores as es
    x = 17                                                       # 1-based, the second nucleotide of the loop
    region = "." * (x - 1) + "x" + "." * (36 - x)
    assert TARGET36[x - 1] == "."
    inp = SimpleNamespace(name="acc36", sec_struct=TARGET36, seq_restr="N" * 36, seed_seq=None, alt_sec_struct=None,
                          alt_sec_structs=None, accessible=region)
    plain = SimpleNamespace(**dict(vars(inp), accessible=None))
    w = 2.5
    kw = dict(replicas=4, exchange=5, steps=2, seed=11)
    res = design.run_design_fast(inp, accessible_weight=w, **kw)
    assert res["used_native_loop"] is False
    recs = res["simulation_data"]
    assert len(recs) == 4 * 3 and all("opening_energy" in r and "p_unpaired" in r for r in recs)
    rows = recs + [vars(res["best"])]
    ref = {s: oracle.pf_forbid(s, x, 0) - oracle.pf(s) for s in {r["sequence"] for r in rows}}
    for r in rows:
        assert abs(r["opening_energy"] - ref[r["sequence"]]) <= TOL, (r["sequence"], r["opening_energy"], ref[r["sequence"]])
        assert abs(r["p_unpaired"] - np.exp(-r["opening_energy"] / engine.KT)) <= 1e-12
    assert max(ref.values()) > 0.0
    # the scoring function is that of the same candidates without the block, plus w Eopen
    eng, hk = res["engine"], engine.HostKernels()
    eng.set_targets([TARGET36])
    seqs = sorted(ref)
    u8 = np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1)
    by_seq = {}
    for k0 in range(0, len(seqs), eng.max_R):                    # (the run's engine holds its four replicas)
        base = es.score_arrays(eng, hk, TARGET36, es.parse_scoring_functions("Ed-Epf:1.0"), u8[k0:k0 + eng.max_R])
        by_seq.update({s: float(base.score[k]) for k, s in enumerate(seqs[k0:k0 + eng.max_R])})
    for r in rows:
        assert abs(r["scoring_function"] - (by_seq[r["sequence"]] + w * r["opening_energy"])) <= 1e-9
    assert "opening_energy" not in design.run_design_fast(plain, **kw)["simulation_data"][0]
