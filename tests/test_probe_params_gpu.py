"""GPU parity under the probe parameter sets of tests/probe_params.py: one engine built on the "distinct" blob against the
oracle on the same blob (pinned to enumeration by tests/test_probe_params_oracle.py).  Every other GPU test runs on
Turner-1999, which cannot tell the three interior mismatch tables apart, nor mmM from mmExt or d5 + d3, nor eMLb from scale,
and which has no triloop and no hexaloop; this module is where the compiled kernels, the fused launch, the host's table staging
and the native Monte-Carlo loops meet a second table set.  Shapes are the smallest that reach each path."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import pyoracle
from tests import constructs as C
from tests import probe_params as PP
from tests.test_gpu_parity import EDEF_TOL, EPF_TOL_ORACLE
from tests.test_loop_constructs_gpu import _options
from tests.test_self_dimer_gpu import F4_TOL

pytestmark = pytest.mark.gpu

INF_REF = 10000000
COUNTERS = ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored")


@pytest.fixture(scope="module")
def orc():
    pyoracle.build()
    return pyoracle.Oracle(PP.probe_blob("distinct"))


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=16, max_L=400, device=0, params=PP.probe_blob("distinct"))
    yield e
    e.close()


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), n))


def _records(oracle):
    """the construct families, thinned: the interior shapes and small loops of tests/test_loop_constructs_emulated.py (chosen by
    the Turner-1999 oracle, as there), every hairpin length and special loop, the multiloops, the probe's own sequences"""
    from tests.test_loop_constructs_emulated import _records as base
    recs = base(oracle) + C.hairpin()[::7] + C.multiloop() + C.multiloop(pinned=False)
    for nm, (s, t) in (("probe_tri", PP.TRI_HAIRPIN), ("probe_hexa", PP.HEXA_HAIRPIN), ("probe_multiloop", PP.MULTILOOP)):
        recs.append(C.Record(nm, "probe", s, t, (0, len(s) - 1)))
    for loops in (PP.TRILOOPS, PP.HEXALOOPS):
        for e, _ in loops:
            s, t = PP.special_hairpin(e)
            recs.append(C.Record("probe_" + e, "probe", s, t, (4, len(s) - 5)))
    return recs


def _score(eng, seqs, targets, pk=False):
    from desirna_amd import engine as E
    eng.set_targets(targets)
    return eng.score_batch(seqs, E.NEED_PF | E.NEED_MFE | E.NEED_EVAL | (E.NEED_PK if pk else 0))


def _against_oracle(orc, out, seqs, targets, pk=False, label=""):
    for k, s in enumerate(seqs):
        ss, e = orc.mfe(s)
        want = orc.pk_struct(s, ss) if pk else ss
        assert (out["mfe_ss"][k], int(out["Emfe"][k])) == (want, e), (label, s)
        assert abs(float(out["Epf"][k]) - orc.pf(s)) < EPF_TOL_ORACLE, (label, s)
        for t, tg in enumerate(targets):
            assert int(out["Ed"][k, t]) == orc.eval_structure(s, tg), (label, s, tg)


@pytest.mark.parametrize("L,k", [(72, 0), (100, 11)])
def test_construct_families(eng, orc, oracle, L, k):
    """every record in a poly-A frame of 72 nt (LDS kernels) and 100 nt (two-workgroup folds), its own target the eval target"""
    frames = [C.pad(r, L, k) for r in _records(oracle) if len(r.sequence) <= L]
    assert len(frames) >= 70
    for b in range(0, len(frames), 16):
        sub = frames[b:b + 16]
        seqs, tgts = [f[0] for f in sub], [f[1] for f in sub]
        out = _score(eng, seqs, tgts)
        for i, s in enumerate(seqs):
            ss, e = orc.mfe(s)
            assert (out["mfe_ss"][i], int(out["Emfe"][i])) == (ss, e), s
            assert abs(float(out["Epf"][i]) - orc.pf(s)) < EPF_TOL_ORACLE, s
            assert int(out["Ed"][i, i]) == orc.eval_structure(s, tgts[i]), s


@pytest.mark.parametrize("L", [12, 36, 64, 65, 100, 200])
def test_random_batches_under_every_launch_setting(eng, orc, L):
    """R = 4, the last sequence G/C only; dual 0 / 2, pf_helper 0 / 1, fused 0 / 1: integers and strings equal across the
    settings, Epf bit-equal across dual and pf_helper and to 1e-9 across fused; the first setting against the oracle (with pk)"""
    rng = np.random.default_rng(4400 + L)
    seqs = [_rand(rng, L) for _ in range(3)] + [_rand(rng, L, "GC")]
    tgts = [orc.mfe(seqs[0])[0], "." * L]
    ref = None
    for fused in (0, 1):
        for dual in (0, 2):
            for helper in (0, 1):
                with _options(eng, dual=dual, pf_helper=helper, fused=fused):
                    out = _score(eng, seqs, tgts, pk=True)
                if ref is None:
                    ref, ref_fused = out, fused
                    _against_oracle(orc, out, seqs, tgts, pk=True, label=L)
                    continue
                assert out["mfe_ss"] == ref["mfe_ss"] and (out["Emfe"] == ref["Emfe"]).all() and (out["Ed"] == ref["Ed"]).all(), (L, fused, dual, helper)
                if fused == ref_fused:
                    assert out["Epf"].tobytes() == ref["Epf"].tobytes(), (L, fused, dual, helper)
                else:
                    assert np.abs(out["Epf"] - ref["Epf"]).max() < 1e-9, (L, fused, dual, helper)
                if (fused, dual, helper) == (1, 2, 1) and L >= 100:
                    # the fused launch took place (it needs both helpers, so 95 nt and more): four workgroups per sequence
                    with _options(eng, dual=dual, pf_helper=helper, fused=fused):
                        one = _score(eng, seqs, tgts)
                        assert eng.get_option("last_fused") == 1 and eng.get_option("last_workgroups") == 4 * len(seqs), L
                    _against_oracle(orc, one, seqs, tgts, label=(L, "fused"))
                if fused and (dual, helper) == (0, 0):
                    fref = out
                elif fused:
                    assert out["Epf"].tobytes() == fref["Epf"].tobytes(), (L, dual, helper)


@pytest.mark.parametrize("L,pk", [(201, False), (241, True), (361, False)])
def test_strips(eng, orc, L, pk):
    """two, three and four strips per fold (the last with the blocked MFE splits and the tile-product PF sums) against the
    general kernels (strips = 0) and the oracle"""
    rng = np.random.default_rng(4500 + L)
    s, t = PP.MULTILOOP
    head = PP.special_hairpin("GAAAC")[0] + "AAA" + s
    seqs = [_rand(rng, L), head + _rand(rng, L - len(head), "GGCCAU")]
    tgts = [orc.mfe(seqs[0])[0]]
    out = _score(eng, seqs, tgts, pk=pk)
    wgs = eng.get_option("last_workgroups")
    assert wgs == 2 * len(seqs) * {201: 2, 241: 3, 361: 4}[L], wgs
    with _options(eng, strips=0):
        gen = _score(eng, seqs, tgts, pk=pk)
    assert out["mfe_ss"] == gen["mfe_ss"] and (out["Emfe"] == gen["Emfe"]).all() and (out["Ed"] == gen["Ed"]).all()
    assert np.abs(out["Epf"] - gen["Epf"]).max() < EPF_TOL_ORACLE
    _against_oracle(orc, out, seqs, tgts, pk=pk, label=L)


def test_ragged_call_equals_the_per_length_calls(eng, orc):
    rng = np.random.default_rng(4600)
    seqs = [_rand(rng, L) for L in (361, 241, 130, 36)]
    tgts = [orc.mfe(s)[0] for s in seqs]
    eng.set_targets_ragged(tgts)
    out = eng.score_ragged(seqs, list(range(4)))
    for k, s in enumerate(seqs):
        one = _score(eng, [s], [tgts[k]])
        assert (out["mfe_ss"][k], int(out["Emfe"][k]), int(out["Ed"][k])) == (one["mfe_ss"][0], int(one["Emfe"][0]), int(one["Ed"][0, 0])), len(s)
        assert abs(float(out["Epf"][k]) - float(one["Epf"][0])) < EPF_TOL_ORACLE, len(s)
        assert (out["mfe_ss"][k], int(out["Emfe"][k])) == orc.mfe(s) and int(out["Ed"][k]) == orc.eval_structure(s, tgts[k]), len(s)
        assert abs(float(out["Epf"][k]) - orc.pf(s)) < EPF_TOL_ORACLE, len(s)


@pytest.mark.parametrize("lds", [1, 0])
def test_ensemble_defect_and_pair_probabilities(eng, orc, lds):
    M = eng.get_option("edef_lds_max")
    rng = np.random.default_rng(4700)
    for L in sorted({9, 36, M, M + 1, 100}):
        seqs = [_rand(rng, L), _rand(rng, L, "GGCCAU")] + ([C.pad(C.Record("m", "m", *PP.MULTILOOP, (0, 20)), L, 3)[0]] if L >= 21 else [PP.TRI_HAIRPIN[0]])
        for tg in (orc.mfe(seqs[0])[0], "." * L):
            with _options(eng, edef_lds=lds):
                eng.set_targets([tg])
                ed, bpp = eng.ensemble_defect(seqs, want_bpp=True)
            for k, s in enumerate(seqs):
                oe, ob = orc.ensemble_defect(s, tg, want_bpp=True)
                assert abs(ed[k] - oe) < EDEF_TOL and np.abs(bpp[k] - ob).max() < EDEF_TOL, (L, lds, s)


@pytest.mark.parametrize("lds", [1, 0])
def test_second_best_energy_and_ranked_structures(eng, orc, lds):
    M = eng.get_option("subopt_lds_max")
    rng = np.random.default_rng(4800)
    for L in sorted({20, M, M + 1}):
        seqs = [_rand(rng, L), _rand(rng, L, "GGCCAU"), C.pad(C.Record("m", "m", *PP.MULTILOOP, (0, 20)), L, 5)[0] if L >= 21 else _rand(rng, L, "GC")]
        with _options(eng, subopt_lds=lds):
            E2, E12 = eng.subopt_energy(seqs, want_both=True)
            ranked = [eng.subopt_structs(seqs, K) for K in (4, 8)]
        for k, s in enumerate(seqs):
            two = orc.two_best(s)
            assert tuple(int(x) for x in E12[k]) == two and int(E2[k]) == orc.subopt_energy(s), (L, lds, s)
            for (En, ss), K in zip(ranked, (4, 8)):
                e = [int(x) for x in En[k]]
                assert len(e) == K and e == sorted(e) and tuple(e[:2]) == two, (L, K, s)
                live = [x for x, v in zip(ss[k], e) if v < INF_REF]
                assert len(set(live)) == len(live), (L, K, s)
                for x, v in zip(ss[k], e):
                    if v < INF_REF:
                        assert orc.eval_structure(s, x) == v, (L, K, s, x)


def _pairs(eng):
    M, ME = eng.get_option("cofold_lds_max"), eng.get_option("cofold_edef_lds_max")
    shapes = [(17, 18), (32, 32), (M // 2 + 1, M - M // 2), (ME // 2, ME - ME // 2), (ME // 2, ME - ME // 2 + 1)]
    assert sum(shapes[2]) == M + 1 and sum(shapes[3]) == ME and sum(shapes[4]) == ME + 1
    return shapes


def _join_target(la, lb, k=4):
    return "." * (la - k - 1) + "(" * k + "." + "&" + "." + ")" * k + "." * (lb - k - 1)


def test_two_strands(eng, orc):
    """co-fold MFE, the four free energies and E(target) with the nick against the oracle under cofold_lds 1 / 0; defect and
    pair probabilities, second-best energy and ranked structures: LDS and general kernels bit for bit, the lowest energy the
    oracle's co-fold MFE, every ranked string worth its energy, the defect the definition on the kernel's matrix, FAB the oracle's"""
    from tests.test_cofold_edef_emulated import defect_from_matrix
    rng = np.random.default_rng(4900)
    for la, lb in _pairs(eng):
        x = _rand(rng, la, "GGCCAU")
        seqs = [_rand(rng, la) + "&" + _rand(rng, lb), x + "&" + (x if la == lb else _rand(rng, lb, "GGCCAU"))]
        tg = _join_target(la, lb)
        flat_t = tg.replace("&", "")
        res = []
        for lds in (1, 0):
            with _options(eng, cofold_lds=lds, edef_lds=lds, subopt_lds=lds):
                eng.set_targets([flat_t])
                co = eng.cofold_batch(seqs)
                ed, bpp = eng.cofold_ensemble_defect(seqs, want_bpp=True)
                E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
                ranked = [eng.cofold_subopt_structs(seqs, K) for K in (4, 8)]
            res.append((ed, bpp, E2, E12, ranked))
            for k, s in enumerate(seqs):
                oss, oe = orc.cofold_mfe(s)
                assert (co["mfe_ss"][k], int(co["Emfe"][k])) == (oss, oe), (s, lds)
                got = [float(co[n][k]) for n in ("FA", "FB", "FcAB", "FAB")]
                assert max(abs(g - o) for g, o in zip(got, orc.cofold_pf(s))) < EPF_TOL_ORACLE, (s, lds)
                assert int(co["Ed"][k, 0]) == orc.eval_structure(s, flat_t, cut=la), (s, lds)
                assert int(E12[k, 0]) == oe and int(E12[k, 0]) <= int(E12[k, 1]), (s, lds)
                assert abs(float(ed[k]) - defect_from_matrix(bpp[k], tg)) < 1e-12, (s, lds)
                for (En, ss), K in zip(ranked, (4, 8)):
                    e = [int(v) for v in En[k]]
                    assert e == sorted(e) and e[0] == oe and e[1] == int(E12[k, 1]), (s, K, lds)
                    for db, v in zip(ss[k], e):
                        if v < INF_REF:
                            assert orc.eval_structure(s, db.replace("&", ""), cut=la) == v, (s, db)
        (eda, ba, E2a, E12a, ra), (edb, bb, E2b, E12b, rb) = res
        assert E2a.tobytes() == E2b.tobytes() and E12a.tobytes() == E12b.tobytes(), (la, lb)
        assert all(np.asarray(x[0]).tobytes() == np.asarray(y[0]).tobytes() and x[1] == y[1] for x, y in zip(ra, rb)), (la, lb)
        assert np.abs(eda - edb).max() < EDEF_TOL and np.abs(ba - bb).max() < EDEF_TOL, (la, lb)


def test_two_strands_equal_the_emulated_kernels(eng):
    """what the oracle lacks for two strands -- pair probabilities and the defect, the second-best energy, the ranked
    structures -- against the kernel sources compiled for the CPU on the same blob (tests/test_probe_params_emulated.py holds
    those to enumeration on short pairs), with the LDS kernels on and off: probabilities and defect to EDEF_TOL, energies and
    strings exactly.  Two pairs of 17 + 18 nt; one of 32 + 32 nt without the ranked lists, whose emulation takes minutes.
    The emulation jobs run side by side in worker processes."""
    from tests import test_probe_params_emulated as T
    from tests.emu import emu, emu_cofold_kbest
    rng = np.random.default_rng(4950)
    cases = [(_rand(rng, 17) + "&" + _rand(rng, 18), True), (_rand(rng, 17, "GGCCAU") + "&" + _rand(rng, 18, "GGCCAU"), True),
             (_rand(rng, 32) + "&" + _rand(rng, 32), False)]
    D, jobs = "distinct", []
    for s, ranked in cases:
        tg = _join_target(s.index("&"), len(s) - 1 - s.index("&"))
        jobs += [(D, "co_outside", s, tg), (D, "co_second_best", s)] + ([(D, "kbest", s, 4), (D, "kbest", s, 8)] if ranked else [])
    emu.build()
    emu_cofold_kbest.build()
    jobs.sort(key=lambda j: (j[1] != "kbest", -len(j[2])))               # the longest jobs first
    ref = dict(zip(jobs, emu._spawn_map(T._job, jobs, 16)))
    for s, ranked in cases:
        tg = _join_target(s.index("&"), len(s) - 1 - s.index("&"))
        ed_e, bpp_e, F4_e, st_e = ref[(D, "co_outside", s, tg)]
        e2_e, e12_e, st2_e = ref[(D, "co_second_best", s)]
        assert (st_e, st2_e) == (0, 0)
        for lds in (1, 0):
            with _options(eng, cofold_lds=lds, edef_lds=lds, subopt_lds=lds):
                eng.set_targets([tg.replace("&", "")])
                ed, bpp = eng.cofold_ensemble_defect([s], want_bpp=True)
                E2, E12 = eng.cofold_subopt_energy([s], want_both=True)
                got = [eng.cofold_subopt_structs([s], K) for K in (4, 8)] if ranked else []
            dP, dE = float(np.abs(bpp[0] - bpp_e).max()), abs(float(ed[0]) - ed_e)
            print("%d nt lds=%d: max|dP| %.3e |dEdef| %.3e" % (len(s) - 1, lds, dP, dE))
            assert dP < EDEF_TOL and dE < EDEF_TOL, (s, lds)
            assert (int(E2[0]), (int(E12[0, 0]), int(E12[0, 1]))) == (e2_e, e12_e), (s, lds)
            for (En, ss), K in zip(got, (4, 8)):
                Ee, sse, stk = ref[(D, "kbest", s, K)]
                assert stk == 0 and ([int(v) for v in En[0]], list(ss[0])) == (Ee, sse), (s, K, lds)


def test_self_dimer(eng, orc):
    M = eng.get_option("self_dimer_lds_max")
    rng = np.random.default_rng(5000)
    for L in (M, M + 1):
        seqs = [_rand(rng, L, "GGCCAU"), C.selfdimer()[7].sequence + _rand(rng, L - len(C.selfdimer()[7].sequence))]
        out = []
        for lds in (1, 0):
            with _options(eng, self_dimer_lds=lds):
                out.append(eng.self_dimer(seqs))
        for n in ("FA", "FcAA", "FAA", "oligo_fraction"):
            assert out[0][n].tobytes() == out[1][n].tobytes(), (L, n)
        for k, s in enumerate(seqs):
            o = orc.cofold_pf(s + "&" + s)
            assert max(abs(float(out[0][n][k]) - o[c]) for n, c in (("FA", 0), ("FcAA", 2), ("FAA", 3))) < F4_TOL, (L, s)


# ---- the native Monte-Carlo loops: their own scoring calls under a second table set

def _input(name, structure, restr=None):
    return SimpleNamespace(name=name, sec_struct=structure, seq_restr=restr or "N" * len(structure.replace("&", "")), seed_seq=None,
                           alt_sec_struct=None, alt_sec_structs=None)


def _same_value(x, y, exact):
    if isinstance(x, float) and not exact:
        return abs(x - y) < 1e-9           # native against per-iteration loop: as tests/test_nd_native_gpu.py::_three_drivers
    return x == y


def _same_run(a, b, label, exact=False):
    """every field of every record, the counters and every field of `best`"""
    ra, rb = a["simulation_data"], b["simulation_data"]
    assert len(ra) == len(rb) > 0, label
    for x, y in zip(ra, rb):
        assert x.keys() == y.keys(), label
        for k in x:
            assert _same_value(x[k], y[k], exact), (label, k, x[k], y[k])
    for k in COUNTERS:
        assert a["stats"][k] == b["stats"][k], (label, k)
    va, vb = vars(a["best"]), vars(b["best"])
    assert va.keys() == vb.keys() and all(_same_value(va[k], vb[k], exact) for k in va), (label, va, vb)
    assert a["steps"] == b["steps"] and a["solved"] == b["solved"], label


# the Standard example's target with a solved sequence under the probe as well, and the restraints under which the run starts
# from it (tests/test_nd_native_gpu.py): the first iteration already folds second-best structures
TARGET36 = "((((((.((((((((....))))).)).).))))))"
NATIVE = {"mc_run": dict(), "nd": dict(negative_design="on"), "oa": dict(oligo="on"), "edef": dict(scoring_f="Ed-Epf:0.5,Edef:1.0")}


@pytest.mark.parametrize("loop", sorted(NATIVE))
def test_native_loop_equals_the_per_iteration_loop(eng, orc, loop):
    """R = 4, two exchange steps from a solved start: the native loop against the host loop that scores through the engine's
    Python calls, every field of the records (subopt_e and esubopt_minus_Epf with -nd on, oligo_fraction with -oa on)"""
    from desirna_amd import design
    from tests.test_nd_native_gpu import STD_RESTR, STD_SOLVED
    assert orc.mfe(STD_SOLVED)[0] == TARGET36                    # solved under the probe, too
    inp = _input("probe36", TARGET36, STD_RESTR)
    kw = dict(replicas=4, exchange=10, steps=2, seed=5, engine=eng, **NATIVE[loop])
    nat = design.run_design_fast(inp, native_loop=True, **kw)
    per = design.run_design_fast(inp, native_loop=False, **kw)
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    _same_run(nat, per, loop)
    first = nat["simulation_data"][:4]
    assert all(r["sequence"] == STD_SOLVED and r["mcc"] == 0 for r in first)
    if loop == "nd":
        assert all(r["subopt_e"] != 0 for r in first)
        for r in nat["simulation_data"]:
            if r["mcc"] == 0:                                    # the second-best energy the loop took is the oracle's
                assert abs(r["subopt_e"] - orc.subopt_energy(r["sequence"]) / 100.0) < 1e-9, r["sequence"]
    if loop == "oa":
        assert all("oligo_fraction" in r for r in nat["simulation_data"])
        for r in first:                                          # ... and is what the self-dimer call gives (test_self_dimer: the oracle's)
            assert abs(r["oligo_fraction"] - float(eng.self_dimer([r["sequence"]])["oligo_fraction"][0])) < 1e-12


def test_native_cofold_loop_equals_the_per_iteration_loop(eng, example_inputs):
    from desirna_amd import design
    ex = example_inputs["RNA_RNA_complex_design_input"]
    inp = SimpleNamespace(name=ex["name"][0], sec_struct=ex["sec_struct"][0], seq_restr=ex["seq_restr"][0], seed_seq=None,
                          alt_sec_struct=None, alt_sec_structs=None)
    kw = dict(replicas=4, exchange=10, steps=2, seed=5, engine=eng, scoring_f="Ed-Epf:0.9")
    nat = design.run_design_fast(inp, native_loop=True, **kw)
    per = design.run_design_fast(inp, native_loop=False, **kw)
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    _same_run(nat, per, "cofold")


def test_puzzle_batch_equals_the_fast_driver_per_puzzle(eng, eterna_targets):
    """three short puzzles in lock-step against the native loop per puzzle: equal, as tests/test_puzzle_set_gpu.py has it"""
    from desirna_amd import design
    names = [n for n in eterna_targets if len(eterna_targets[n]) <= 40][:3]
    inputs = [_input(n, eterna_targets[n]) for n in names]
    assert len(inputs) == 3 and len({len(i.sec_struct) for i in inputs}) >= 2
    kw = dict(replicas=4, exchange=10, steps=2, seed=5, engine=eng)
    got = design.run_puzzle_batch(inputs, **kw)
    for inp, a in zip(inputs, got):
        b = design.run_design_fast(inp, **kw)
        assert a["used_native_loop"] is True and b["used_native_loop"] is True
        _same_run(a, b, inp.name, exact=True)


# ---- the special-loop tables at their capacity

def test_full_special_tables_and_one_entry_too_many():
    """64 triloops, 64 tetraloops, 64 hexaloops: hairpins closed by the first and the last entry of each list through MFE, PF,
    eval and the ensemble defect.  65 tetraloops: EngineError -2, and a fresh engine works"""
    from desirna_amd import engine as E
    blob = PP.probe_blob("full_special")
    orc = pyoracle.Oracle(blob)
    eng = E.Engine(max_R=4, max_L=40, device=0, params=blob)
    try:
        for lst in PP.special_loops("full_special"):
            pair = [PP.special_hairpin(lst[k][0]) for k in (0, len(lst) - 1)]
            seqs, tgts = [p[0] for p in pair], [p[1] for p in pair]
            assert tgts[0] == tgts[1]
            out = _score(eng, seqs, tgts[:1])
            _against_oracle(orc, out, seqs, tgts[:1])
            ed, bpp = eng.ensemble_defect(seqs, want_bpp=True)
            for k, s in enumerate(seqs):
                oe, ob = orc.ensemble_defect(s, tgts[0], want_bpp=True)
                assert abs(ed[k] - oe) < EDEF_TOL and np.abs(bpp[k] - ob).max() < EDEF_TOL, s
    finally:
        eng.close()
    with pytest.raises(E.EngineError) as ei:
        E.Engine(max_R=4, max_L=40, device=0, params=PP.probe_blob("too_many_tetraloops"))
    assert ei.value.code == -2
    eng = E.Engine(max_R=4, max_L=40, device=0, params=blob)
    try:
        s, t = PP.special_hairpin(PP.special_loops("full_special")[1][-1][0])
        _against_oracle(orc, _score(eng, [s], [t]), [s], [t])
    finally:
        eng.close()
