"""Two-strand designs on the GPU: the short-pair co-fold kernels (tables in LDS, option cofold_lds) against the general ones and
the oracle, and the native two-strand Monte-Carlo loop against the per-iteration loop and the Python driver."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPF_TOL_ORACLE = 1e-9   # kcal/mol, fp64 summation-order differences only
EPF_TOL_GOLDEN = 2e-6   # kcal/mol, goldens are float32
RUNS = ("RNA_RNA_complex_design_input", "Homodimer_design_input")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng400():
    from desirna_amd import engine as E
    e = E.Engine(max_R=128, max_L=400)
    yield e
    e.close()


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _both_paths(eng, seqs):
    out = []
    for lds in (1, 0):
        eng.set_option("cofold_lds", lds)
        assert eng.get_option("cofold_lds") == lds
        out.append(eng.cofold_batch(seqs))
    eng.set_option("cofold_lds", 1)
    return out


def _same(a, b, bits=False):
    assert a["mfe_ss"] == b["mfe_ss"]
    assert (a["Emfe"] == b["Emfe"]).all() and (a["Ed"] == b["Ed"]).all()
    if bits:
        for k in ("FA", "FB", "FcAB", "FAB"):
            assert a[k].tobytes() == b[k].tobytes(), k


def test_option_default_and_bound(eng400):
    assert eng400.get_option("cofold_lds") == 1
    assert eng400.get_option("cofold_lds_max") >= 64


def test_short_path_equals_general_path_on_golden_rows(eng400, traj_golden, example_inputs):
    for run in RUNS:
        rows = [r for r in traj_golden if r["run"] == run][:128]
        eng400.set_targets([example_inputs[run]["sec_struct"][0].replace("&", "")])
        assert len(rows[0]["sequence"]) - 1 <= eng400.get_option("cofold_lds_max")
        a, b = _both_paths(eng400, [r["sequence"] for r in rows])
        _same(a, b, bits=True)                         # same candidates, same order of summation: the same bits
        for k, r in enumerate(rows):
            assert a["mfe_ss"][k] == r["mfe_ss"]
            assert abs(float(a["FAB"][k]) - float(r["Epf"])) < EPF_TOL_GOLDEN, r["sequence"]
            assert int(a["Ed"][k, 0]) == round(float(r["edesired"]) * 100)


def test_both_paths_against_the_oracle(eng400, oracle):
    rng = np.random.default_rng(31)
    M = eng400.get_option("cofold_lds_max")
    for la, lb in ((1, 1), (2, 5), (17, 18), (25, 11), (1, M - 1), (M - 1, 1), (M // 2, M // 2)):
        seqs = [_rand(rng, la) + "&" + _rand(rng, lb) for _ in range(3)] + [_rand(rng, la, "GC") + "&" + _rand(rng, lb, "GC"),
                                                                           "A" * la + "&" + "A" * lb]
        if la == lb:
            a = _rand(rng, la)
            seqs.append(a + "&" + a)
        eng400.set_targets(["." * (la + lb)])
        for out in _both_paths(eng400, seqs):
            for k, s in enumerate(seqs):
                assert (out["mfe_ss"][k], int(out["Emfe"][k])) == oracle.cofold_mfe(s), s
                got = [float(out[x][k]) for x in ("FA", "FB", "FcAB", "FAB")]
                assert max(abs(g - o) for g, o in zip(got, oracle.cofold_pf(s))) < EPF_TOL_ORACLE, s


def test_short_path_bits_do_not_depend_on_batch_or_engine(eng400):
    from desirna_amd import engine as E
    rng = np.random.default_rng(7)
    seqs = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(64)]
    eng400.set_targets(["." * 36])
    full = eng400.cofold_batch(seqs)
    one = eng400.cofold_batch(seqs[5:6])
    small = E.Engine(max_R=64, max_L=36)
    try:
        small.set_targets(["." * 36])
        other = small.cofold_batch(seqs)
    finally:
        small.close()
    for k in ("FA", "FB", "FcAB", "FAB"):
        assert one[k][0].tobytes() == full[k][5].tobytes()
        assert other[k].tobytes() == full[k].tobytes()
    assert other["mfe_ss"] == full["mfe_ss"] and one["mfe_ss"][0] == full["mfe_ss"][5]


def test_pair_beyond_the_bound_takes_the_general_kernels(eng400, oracle):
    rng = np.random.default_rng(8)
    M = eng400.get_option("cofold_lds_max")
    seqs = [_rand(rng, M // 2 + 1) + "&" + _rand(rng, M // 2) for _ in range(4)]
    eng400.set_targets(["." * (M + 1)])
    a, b = _both_paths(eng400, seqs)
    _same(a, b, bits=True)
    assert (a["mfe_ss"][0], int(a["Emfe"][0])) == oracle.cofold_mfe(seqs[0])


def test_bad_letter_and_status_words(eng400):
    from desirna_amd import engine as E
    eng400.set_targets(["." * 16])
    for lds in (1, 0):
        eng400.set_option("cofold_lds", lds)
        with pytest.raises(E.EngineError) as ei:
            eng400.cofold_batch(["GGGAAACC&GGUUUCCC", "GGGANACC&GGUUUCCC"])
        assert ei.value.code == -4 and "sequence 1" in str(ei.value)
    eng400.set_option("cofold_lds", 1)


def _inp(example_inputs, run):
    ex = example_inputs[run]
    return SimpleNamespace(name=ex["name"][0], sec_struct=ex["sec_struct"][0], seq_restr=ex["seq_restr"][0], seed_seq=None,
                           alt_sec_struct=None, alt_sec_structs=None)


@pytest.mark.parametrize("run,dimer,sf", [("RNA_RNA_complex_design_input", "off", "Ed-Epf:0.9"),
                                          ("Homodimer_design_input", "on", "Ed-Epf:0.9"),
                                          ("RNA_RNA_complex_design_input", "off", "Ed-Epf:0.5,Edef:1.0")])
def test_native_loop_equals_per_iteration_loop_equals_python_driver(example_inputs, run, dimer, sf, monkeypatch):
    from desirna_amd import design
    from desirna_amd import energy_scores as es
    if "," in sf:          # more than one -sf term: the reference keeps the first only (parse_scoring_functions); all of them here
        monkeypatch.setattr(es, "parse_scoring_functions", lambda s, first_term_only=True, _p=es.parse_scoring_functions: _p(s, False))
    inp = _inp(example_inputs, run)
    kw = dict(replicas=8, exchange=10, steps=3, seed=4, scoring_f=sf, dimer=dimer)
    nat = design.run_design_fast(inp, native_loop=True, **kw)
    per = design.run_design_fast(inp, native_loop=False, **kw)
    py = design.run_design(inp, **kw)
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    rn, rp, ry = nat["simulation_data"], per["simulation_data"], py["simulation_data"]
    assert len(rn) == len(rp) == len(ry) == 8 * 4
    for other in (rp, ry):
        assert [r["sequence"] for r in rn] == [r["sequence"] for r in other]
        assert [r["temp_shelf"] for r in rn] == [r["temp_shelf"] for r in other]
        assert [r["mfe_ss"] for r in rn] == [r["mfe_ss"] for r in other]
        for x, y in zip(rn, other):
            assert abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
            assert abs(x["oligo_fraction"] - y["oligo_fraction"]) < 1e-9
    assert all("&" in r["sequence"] and "&" in r["mfe_ss"] and "oligomer_bonus" in r for r in rn)
    for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
        assert nat["stats"][k] == per["stats"][k] == py["stats"][k], k
    assert nat["best"].sequence == per["best"].sequence == py["best"].sequence
    for e in (nat["engine"], per["engine"], py["engine"]):
        e.close()


def test_mc_run_cofold_argument_errors(example_inputs):
    from desirna_amd import engine as E
    from desirna_amd import design
    inp = _inp(example_inputs, "RNA_RNA_complex_design_input")
    prob = design.DesignProblem(inp.sec_struct, inp.seq_restr)
    Ls, R = prob.n, 2
    cut = inp.sec_struct.index("&")
    eng = E.Engine(max_R=R, max_L=Ls - 1)
    hk = E.HostKernels()
    try:
        seq = prob.initial_sequence(__import__("random").Random(1))
        state = dict(seqs=np.frombuffer((seq * R).encode(), np.uint8).reshape(R, Ls).copy(),
                     mfe_ss=np.frombuffer(("." * cut + "&" + "." * (Ls - cut - 1)).encode() * R, np.uint8).reshape(R, Ls).copy(),
                     score=np.zeros(R), mcc1=np.ones(R), Epf=np.zeros(R), Ed=np.zeros(R), oligo_fraction=np.zeros(R), bonus=np.zeros(R))
        best = dict(seq=state["seqs"][0].copy(), ss=state["mfe_ss"][0].copy(), vals=np.zeros(6))
        args = lambda sf: (prob, "heterodimer", 1, np.zeros(R, np.int32), R, 0.7, 0.0, True, np.array([10.0, 20.0]), sf,
                           hk.rng_seed(np.arange(R)), state, np.zeros(3, np.int64), best)
        with pytest.raises(E.EngineError) as ei:                  # no targets installed
            eng.mc_run_cofold(*args([("Ed-Epf", 1.0)]))
        assert ei.value.code == -1 and "drna_set_targets" in str(ei.value)
        eng.set_targets([inp.sec_struct.replace("&", "")])
        eng.TERM_IDS = dict(E.Engine.TERM_IDS, bogus=9)
        with pytest.raises(E.EngineError) as ei:                  # unknown term id
            eng.mc_run_cofold(*args([("bogus", 1.0)]))
        assert ei.value.code == -1 and "unknown scoring term" in str(ei.value)
        p = lambda a: a.ctypes.data
        ids, ws, sh, tt = np.zeros(1, np.int32), np.ones(1), np.zeros(R, np.int32), np.array([10.0, 20.0])
        am = E.co_allowed_mask(prob)
        for bad_cut in (0, Ls - 1):                               # cut outside [1, L - 1]
            rc = eng._L.drna_mc_run_cofold(eng._h, R, Ls - 1, bad_cut, 1, inp.sec_struct.encode(), p(am), 1, p(sh), R, 0.7, 0.0, 1,
                                           p(tt), 504.12, 1, p(ids), p(ws), p(hk.rng_seed(np.arange(R))), p(state["seqs"]),
                                           p(state["mfe_ss"]), p(state["score"]), p(state["mcc1"]), p(state["Epf"]), p(state["Ed"]),
                                           p(state["oligo_fraction"]), p(state["bonus"]), p(np.zeros(3, np.int64)), p(best["seq"]),
                                           p(best["ss"]), p(best["vals"]))
            assert rc == -1 and b"cut" in eng._L.drna_last_error(eng._h)
    finally:
        eng.close()


def test_two_strands_with_alternative_structures_raise(example_inputs):
    from desirna_amd import design
    inp = _inp(example_inputs, "RNA_RNA_complex_design_input")
    inp.alt_sec_struct, inp.alt_sec_structs = inp.sec_struct, [inp.sec_struct]
    with pytest.raises(NotImplementedError):
        design.run_design_fast(inp, replicas=2, exchange=1, steps=1)


def test_cli_two_strand_input_takes_the_native_driver(example_inputs, tmp_path):
    from desirna_amd import design
    inp = _inp(example_inputs, "RNA_RNA_complex_design_input")
    f = tmp_path / "pair.txt"
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (inp.name, inp.seq_restr, inp.sec_struct))
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-R", "8", "-e", "10", "-s", "3", "-seed", "4",
                          "-o", str(out)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr
    names = os.listdir(out)
    for suffix in ("_results.csv", "_traj.csv", "_stats", "_best_str"):
        assert any(n.endswith(suffix) for n in names), (suffix, names)
    ref = design.run_design(inp, replicas=8, exchange=10, steps=3, seed=4)
    ref["engine"].close()
    assert res.stdout.splitlines()[1] == ref["best"].sequence
