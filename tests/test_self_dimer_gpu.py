"""Avoid oligomerization (-oa on) on the GPU: the self-dimer partition function (fold_self_dimer.hpp, drna_self_dimer_batch) against
the general co-fold kernels on s & s (an engine sized for 2 L) and the oracle, and the self-dimer step of the native Monte-Carlo
loop (drna_mc_run_oa) against the per-iteration loop."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F4_TOL = 1e-9
HAIRPIN14 = "((((......))))"
STD = "Standard_design_input"
COUNTERS = ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored")


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine as E
    e = E.Engine(max_R=8, max_L=100)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    """the parent's way to the same numbers: cofold_batch(s & s) needs 2 L"""
    from desirna_amd import engine as E
    e = E.Engine(max_R=8, max_L=200)
    yield e
    e.close()


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _f4(out):
    return np.stack([out["FA"], out["FA"], out["FcAA"], out["FAA"]], axis=1)


def test_option_default_and_bound(eng):
    from desirna_amd import engine as E
    assert eng.get_option("self_dimer_lds") == 1
    assert eng.get_option("self_dimer_lds_max") >= 36          # the reference's standard example takes the LDS path
    with pytest.raises(E.EngineError):
        eng.set_option("self_dimer_lds_max", 10)               # read-only
    ws = eng.info()["workspace_bytes"]
    eng.self_dimer(["GGAUCACGUA" * 10])                        # the workspace kernel: no allocation of its own
    assert eng.info()["workspace_bytes"] == ws


def test_against_the_general_cofold_kernels_and_the_oracle(eng, eng2, oracle):
    from desirna_amd import engine as E
    from desirna_amd import energy_scores as es
    rng = np.random.default_rng(61)
    M = eng.get_option("self_dimer_lds_max")
    worst = 0.0
    for L in (5, 14, 25, M, M + 1, 100):
        seqs = [_rand(rng, L) for _ in range(6)] + [_rand(rng, L, "GC"), "A" * L]
        out = eng.self_dimer(seqs)
        co = eng2.cofold_batch([s + "&" + s for s in seqs], E.NEED_PF)
        G = np.stack([co["FA"], co["FB"], co["FcAB"], co["FAB"]], axis=1)
        S = np.stack([out["FA"], out["FA"], out["FcAA"], out["FAA"]], axis=1)
        d = float(np.abs(S - G)[:, (0, 2, 3)].max())           # (FB of the general kernel is FA summed from the other end)
        assert float(np.abs(S - G)[:, 1].max()) < F4_TOL, L
        worst = max(worst, d)
        print("L", L, "largest difference to drna_cofold_batch(s & s)", d)
        assert d < F4_TOL, L
        for k, s in enumerate(seqs):
            o = oracle.cofold_pf(s + "&" + s)
            assert max(abs(S[k, c] - o[c]) for c in (0, 2, 3)) < F4_TOL, s
            with np.errstate(invalid="ignore"):
                fw = float(es.oligo_fraction(o[0], o[1], o[2]))
            fg = float(out["oligo_fraction"][k])
            assert (np.isnan(fw) and np.isnan(fg)) or abs(fg - fw) < 3 * 1.7 * F4_TOL, s
        assert out["FcAA"][-1] == 999.0                        # poly-A cannot pair
    print("largest difference over all lengths", worst, "(0.0 = bit-identical)")


def test_lds_and_workspace_kernels_bit_identical(eng):
    rng = np.random.default_rng(62)
    M = eng.get_option("self_dimer_lds_max")
    for L in (5, 14, 25, 36, M):
        seqs = [_rand(rng, L) for _ in range(8)]
        out = []
        for lds in (1, 0):
            eng.set_option("self_dimer_lds", lds)
            assert eng.get_option("self_dimer_lds") == lds
            out.append(eng.self_dimer(seqs))
        eng.set_option("self_dimer_lds", 1)
        assert _f4(out[0]).tobytes() == _f4(out[1]).tobytes(), L
        assert out[0]["oligo_fraction"].tobytes() == out[1]["oligo_fraction"].tobytes()


def test_more_sequences_than_max_R_and_batch_independence(eng):
    rng = np.random.default_rng(63)
    for L in (25, 70):                                         # LDS kernel, workspace kernel
        seqs = [_rand(rng, L) for _ in range(21)]              # max_R = 8: three chunks
        big = eng.self_dimer(seqs)
        one = eng.self_dimer(seqs[13:14])
        assert _f4(big)[13].tobytes() == _f4(one)[0].tobytes()
        part = eng.self_dimer(seqs[8:16])
        assert _f4(big)[8:16].tobytes() == _f4(part).tobytes()


def test_bad_letter_is_an_error_on_both_kernels(eng):
    from desirna_amd import engine as E
    for lds in (1, 0):
        eng.set_option("self_dimer_lds", lds)
        with pytest.raises(E.EngineError) as ei:
            eng.self_dimer(["GGGAAACCCA", "GGGANACCCA"])
        assert ei.value.code == -4 and "sequence 1" in str(ei.value)
    eng.set_option("self_dimer_lds", 1)
    with pytest.raises(E.EngineError):
        eng.self_dimer(["A" * 101])                            # longer than max_L


def _inp(example_inputs, which):
    if which == "hairpin14":
        return SimpleNamespace(name=which, sec_struct=HAIRPIN14, seq_restr="N" * 14, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    ex = example_inputs[STD]
    return SimpleNamespace(name=which, sec_struct=ex["sec_struct"][0], seq_restr=ex["seq_restr"][0], seed_seq=None,
                           alt_sec_struct=None, alt_sec_structs=None)


@pytest.mark.parametrize("which", ["hairpin14", "standard36"])
@pytest.mark.parametrize("nd", ["off", "on"])
def test_native_loop_equals_the_per_iteration_loop(example_inputs, which, nd):
    """drna_mc_run_oa against score_arrays(self_dimer=True) + the native proposer and Metropolis, iteration by iteration: the same
    states after every exchange step, the same counters.  Strings, counters, oligo_fraction (the same host function on both
    sides) and subopt_e exactly; what goes through a logarithm (numpy's on one side, libm's on the other) within 1e-9"""
    from desirna_amd import design
    inp = _inp(example_inputs, which)
    kw = dict(replicas=6, exchange=10, steps=3, seed=5, oligo="on", negative_design=nd)
    nat = design.run_design_fast(inp, native_loop=True, **kw)
    per = design.run_design_fast(inp, native_loop=False, **kw)
    for r in (nat, per):
        r["engine"].close()
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    rn, rp = nat["simulation_data"], per["simulation_data"]
    assert len(rn) == 6 * 4
    assert [r["sequence"] for r in rn] == [r["sequence"] for r in rp]
    assert [r["mfe_ss"] for r in rn] == [r["mfe_ss"] for r in rp]
    assert [r["temp_shelf"] for r in rn] == [r["temp_shelf"] for r in rp]
    for x, y in zip(rn, rp):
        assert list(x) == list(y)
        assert x["oligo_fraction"] == y["oligo_fraction"] and 0 < x["oligo_fraction"] < 1
        assert x["Epf"] == y["Epf"] and x["edesired"] == y["edesired"] and x["mcc"] == y["mcc"] and x["subopt_e"] == y["subopt_e"]
        assert abs(x["monomer_bonus"] - y["monomer_bonus"]) < 1e-9 and abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
    for k in COUNTERS:
        assert nat["stats"][k] == per["stats"][k], k
    assert nat["stats"]["acc_mc"] > 0
    bn, bp = nat["best"], per["best"]
    assert bn.sequence == bp.sequence and bn.mfe_ss == bp.mfe_ss and bn.oligo_fraction == bp.oligo_fraction
    assert abs(bn.scoring_function - bp.scoring_function) < 1e-9 and abs(bn.monomer_bonus - bp.monomer_bonus) < 1e-9
    if nd == "on":
        assert bn.subopt_e == bp.subopt_e


def test_mc_run_oa_draws_are_those_of_mc_run(example_inputs):
    """One iteration at a temperature at which every proposal is accepted: the proposals come from the same draws, so both entry
    points leave the same sequences, structures and energies bit for bit, and the -oa score is the plain score + the bonus, added
    last.  (A sequence set that cannot dimerise has FcAA = 999 and the reference's oligo_fraction is 0 / 0 there, so the bonus
    cannot be forced to zero; later iterations draw from streams that a Metropolis draw -- taken only for a worse proposal --
    may have advanced differently.)"""
    from desirna_amd import design, engine as E
    R = 6
    tg = example_inputs[STD]["sec_struct"][0]
    prob = design.DesignProblem(tg, example_inputs[STD]["seq_restr"][0])
    L = prob.n
    eng = E.Engine(max_R=R, max_L=L)
    hk = E.HostKernels()
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL
    try:
        eng.set_targets([tg])
        seq = prob.initial_sequence(random.Random(3))
        seqs = np.frombuffer((seq * R).encode(), np.uint8).reshape(R, L).copy()
        Epf, Emfe, ss, Ed = eng.score_batch_arrays(seqs)
        mcc, _, _ = hk.simscore(tg, ss)
        st0 = dict(seqs=seqs, mfe_ss=ss, score=Ed[:, 0] / 100.0 - Epf, mcc1=1 - mcc, Epf=Epf, Ed=Ed[:, 0] / 100.0)
        out = []
        for oa in (False, True):
            st = {k: v.copy() for k, v in st0.items()}
            if oa:
                st["oligo_fraction"], st["bonus"] = np.zeros(R), np.zeros(R)
            best = dict(seq=st["seqs"][0].copy(), ss=st["mfe_ss"][0].copy(),
                        vals=np.array([2.0, 0.0, 0.0, 0.0] + ([0.0, 0.0] if oa else [])))       # 1 - MCC = 2: any accepted state is better
            counters, rng = np.zeros(3, np.int64), hk.rng_seed(np.arange(R))
            eng.mc_run(prob, 1, np.arange(R, dtype=np.int32), R, 0.7, 0.0, True, np.full(R, 1e300), [("Ed-Epf", 1.0)], flags, rng,
                       st, counters, best, **(dict(self_dimer=True) if oa else {}))
            out.append((st, best, counters))
        (sa, ba, ca), (sb, bb, cb) = out
        assert ca[0] == cb[0] == R and ca[2] == cb[2] == 0
        assert sa["seqs"].tobytes() != st0["seqs"].tobytes()
        for k in ("seqs", "mfe_ss", "mcc1", "Epf", "Ed"):
            assert sa[k].tobytes() == sb[k].tobytes(), k
        assert ((sb["oligo_fraction"] > 0) & (sb["oligo_fraction"] < 1)).all() and (sb["bonus"] > 0).all()
        assert (sa["score"] + sb["bonus"]).tobytes() == sb["score"].tobytes()
        want = eng.self_dimer([bytes(r).decode() for r in sb["seqs"]])["oligo_fraction"]
        assert want.tobytes() == sb["oligo_fraction"].tobytes()
        # the best state, replica by replica in replica order (first strictly better wins), in the two-strand layout
        k = 0
        for r in range(1, R):
            if (sb["mcc1"][r], sb["score"][r]) < (sb["mcc1"][k], sb["score"][k]):
                k = r
        want = [sb[f][k] for f in ("mcc1", "score", "Epf", "Ed", "oligo_fraction", "bonus")]
        assert bb["vals"].shape == (6,) and bb["vals"].tobytes() == np.array(want).tobytes()
        assert bb["seq"].tobytes() == sb["seqs"][k].tobytes() and bb["ss"].tobytes() == sb["mfe_ss"][k].tobytes()
        assert 0 < bb["vals"][4] < 1 and bb["vals"][5] > 0
    finally:
        eng.close()
