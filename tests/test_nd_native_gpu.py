"""Negative design (-nd on) on the GPU: the LDS-resident second-best kernels (option subopt_lds) against the general ones, the
oracle and the CPU emulation, and the negative-design step of the native Monte-Carlo loops against the per-iteration loop and
the Python driver."""
import csv
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = "Standard_design_input"
HOM = "Homodimer_design_input"
# solved sequences of the two examples, and restraints under which DesignProblem.initial_sequence() is that sequence (N where the
# rule "unpaired -> A, first of an unpaired stretch -> G" gives the letter): the run starts solved and can still move
STD_SOLVED, STD_RESTR = "GCCCCGGCCCCCGGCGAAAGCCGGUGGAGGCGGGGC", "GCCCCGGCCCCCGGCNNNNGCCGGUGGNGGCGGGGC"
HOM_SOLVED, HOM_RESTR = "CGGGGAAACGCCGAAAA&GGCGGAAACCCGGAAAA", "CGGGNNNNCGCCNNNNN&GGCGNNNNCCCGNNNNN"
COUNTERS = ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored")


@pytest.fixture(scope="module")
def eng400():
    from desirna_amd import engine as E
    e = E.Engine(max_R=64, max_L=400)
    yield e
    e.close()


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _both_paths(eng, seqs):
    fn = eng.cofold_subopt_energy if "&" in seqs[0] else eng.subopt_energy
    out = []
    for lds in (1, 0):
        eng.set_option("subopt_lds", lds)
        assert eng.get_option("subopt_lds") == lds
        out.append(fn(seqs, want_both=True))
    eng.set_option("subopt_lds", 1)
    return out


def _shapes(M):
    """(first strand, second strand or 0): 36 nt, the bound, one past it (general kernel either way), three pair shapes"""
    return [(36, 0), (M, 0), (M + 1, 0), (18, 18), (1, 35), (35, 1)]


def _batch(rng, la, lb, R):
    return [_rand(rng, la) + ("&" + _rand(rng, lb) if lb else "") for _ in range(R)]


def test_option_default_and_bound(eng400):
    from desirna_amd import engine as E
    assert eng400.get_option("subopt_lds") == 1
    assert eng400.get_option("subopt_lds_max") >= max(64, eng400.get_option("cofold_lds_max"))
    with pytest.raises(E.EngineError):
        eng400.set_option("subopt_lds_max", 10)                    # read-only


def test_lds_path_equals_general_path_and_the_oracle(eng400, oracle):
    rng = np.random.default_rng(41)
    for la, lb in _shapes(eng400.get_option("subopt_lds_max")):
        seqs = _batch(rng, la, lb, 6) + [_rand(rng, la, "GC") + ("&" + _rand(rng, lb, "GC") if lb else ""),
                                         "A" * la + ("&" + "A" * lb if lb else "")]
        (a2, a12), (b2, b12) = _both_paths(eng400, seqs)
        assert a2.tolist() == b2.tolist() and a12.tolist() == b12.tolist(), (la, lb)
        for k, s in enumerate(seqs):
            if lb:
                assert int(a12[k, 0]) == oracle.cofold_mfe(s)[1], s
            else:
                assert tuple(int(x) for x in a12[k]) == oracle.two_best(s) and int(a2[k]) == oracle.subopt_energy(s), s


def test_results_do_not_depend_on_batch_or_engine(eng400):
    from desirna_amd import engine as E
    rng = np.random.default_rng(43)
    small = E.Engine(max_R=64, max_L=36)
    try:
        for la, lb in ((36, 0), (18, 18)):
            seqs = _batch(rng, la, lb, 64)
            fn = (lambda e, s: e.cofold_subopt_energy(s, want_both=True)) if lb else (lambda e, s: e.subopt_energy(s, want_both=True))
            f2, f12 = fn(eng400, seqs)
            o2, o12 = fn(eng400, seqs[5:6])                       # R = 1 against R = 64
            assert int(o2[0]) == int(f2[5]) and o12[0].tolist() == f12[5].tolist()
            s2, s12 = fn(small, seqs)                             # max_L 36 against 400
            assert s2.tolist() == f2.tolist() and s12.tolist() == f12.tolist()
    finally:
        small.close()


def test_gpu_equals_the_emulation(eng400, blob):
    """integers: no tolerance.  (Short shapes: the emulation of one 36-nt fold takes 20 s of CPU time)"""
    from tests.emu import emu_subopt_lds
    emu = emu_subopt_lds.EmuSuboptLds(blob)
    rng = np.random.default_rng(47)
    for seqs in (_batch(rng, 15, 0, 3), _batch(rng, 6, 7, 3)):
        E2, E12, st = emu.second_best(seqs)
        for g2, g12 in _both_paths(eng400, seqs):
            assert not st.any() and g2.tolist() == E2.tolist() and g12.tolist() == E12.tolist()


def test_bad_letter_is_an_error_on_both_paths(eng400):
    from desirna_amd import engine as E
    for lds in (1, 0):
        eng400.set_option("subopt_lds", lds)
        for fn, seqs in ((eng400.subopt_energy, ["GGGAAACCCA", "GGGANACCCA"]), (eng400.cofold_subopt_energy, ["GGGAAC&GUUCCC", "GGGXAC&GUUCCC"])):
            with pytest.raises(E.EngineError) as ei:
                fn(seqs)
            assert ei.value.code == -4 and "sequence 1" in str(ei.value)
    eng400.set_option("subopt_lds", 1)


def _inp(example_inputs, run, restr=None):
    ex = example_inputs[run]
    return SimpleNamespace(name=ex["name"][0], sec_struct=ex["sec_struct"][0], seq_restr=restr or ex["seq_restr"][0], seed_seq=None,
                           alt_sec_struct=None, alt_sec_structs=None)


def _three_drivers(inp, dimer, seed=4):
    from desirna_amd import design
    kw = dict(replicas=8, exchange=20, steps=3, seed=seed, dimer=dimer)
    nat = design.run_design_fast(inp, native_loop=True, negative_design="on", **kw)
    per = design.run_design_fast(inp, native_loop=False, negative_design="on", **kw)
    py = design.run_design(inp, subopt="on", **kw)
    for r in (nat, per, py):
        r["engine"].close()
    assert nat["used_native_loop"] is True and per["used_native_loop"] is False
    rn = nat["simulation_data"]
    assert len(rn) == 8 * 4
    for other in (per["simulation_data"], py["simulation_data"]):
        assert [r["sequence"] for r in rn] == [r["sequence"] for r in other]
        assert [r["mfe_ss"] for r in rn] == [r["mfe_ss"] for r in other]
        assert [r["temp_shelf"] for r in rn] == [r["temp_shelf"] for r in other]
        for x, y in zip(rn, other):
            assert abs(x["scoring_function"] - y["scoring_function"]) < 1e-9
            assert x["subopt_e"] == y["subopt_e"] and abs(x["esubopt_minus_Epf"] - y["esubopt_minus_Epf"]) < 1e-9
    for k in COUNTERS:
        assert nat["stats"][k] == per["stats"][k] == py["stats"][k], k
    assert nat["best"].sequence == per["best"].sequence == py["best"].sequence
    assert nat["best"].mfe_ss == per["best"].mfe_ss == py["best"].mfe_ss
    assert abs(nat["best"].scoring_function - py["best"].scoring_function) < 1e-9
    assert nat["best"].subopt_e == per["best"].subopt_e == py["best"].subopt_e
    return nat


@pytest.mark.parametrize("run,dimer", [(STD, "off"), (HOM, "on")])
def test_three_drivers_walk_the_same_trajectory(example_inputs, run, dimer):
    _three_drivers(_inp(example_inputs, run), dimer)


@pytest.mark.parametrize("run,dimer,solved,restr", [(STD, "off", STD_SOLVED, STD_RESTR), (HOM, "on", HOM_SOLVED, HOM_RESTR)])
def test_three_drivers_from_a_solved_start(example_inputs, run, dimer, solved, restr):
    """every replica starts solved, so the first iteration already folds second-best structures (H > 0)"""
    nat = _three_drivers(_inp(example_inputs, run, restr), dimer)
    first = nat["simulation_data"][:8]
    assert all(r["sequence"] == solved and r["mcc"] == 0 and r["subopt_e"] != 0 for r in first)


def test_three_drivers_when_nothing_is_ever_solved(example_inputs):
    """A-U pairs only: no proposal of this run folds into the target (H stays 0), and -nd on walks the -nd off trajectory"""
    from desirna_amd import design
    tg = example_inputs[STD]["sec_struct"][0]
    inp = _inp(example_inputs, STD, "".join("W" if c in "()" else "N" for c in tg))
    nat = _three_drivers(inp, "off")
    assert all(r["mcc"] > 0 and r["subopt_e"] == 0 and r["esubopt_minus_Epf"] == 0 for r in nat["simulation_data"])
    off = design.run_design_fast(inp, native_loop=True, replicas=8, exchange=20, steps=3, seed=4)
    off["engine"].close()
    assert [(r["sequence"], r["scoring_function"]) for r in off["simulation_data"]] == \
        [(r["sequence"], r["scoring_function"]) for r in nat["simulation_data"]]


def _mc_state(example_inputs, R):
    import random
    from desirna_amd import design, engine as E
    tg = example_inputs[STD]["sec_struct"][0]
    prob = design.DesignProblem(tg, "".join("W" if c in "()" else "N" for c in tg))
    L = prob.n
    eng = E.Engine(max_R=R, max_L=L)
    eng.set_targets([tg])
    seq = prob.initial_sequence(random.Random(3))
    seqs = np.frombuffer((seq * R).encode(), np.uint8).reshape(R, L).copy()
    Epf, Emfe, ss, Ed = eng.score_batch_arrays(seqs)
    mcc, _, _ = E.HostKernels().simscore(tg, ss)
    state = dict(seqs=seqs, mfe_ss=ss, score=Ed[:, 0] / 100.0 - Epf, mcc1=1 - mcc, Epf=Epf, Ed=Ed[:, 0] / 100.0)
    return eng, prob, state


def test_mc_run_nd_without_a_solved_proposal_equals_mc_run_bit_for_bit(example_inputs):
    from desirna_amd import engine as E
    R = 8
    eng, prob, st0 = _mc_state(example_inputs, R)
    hk = E.HostKernels()
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL
    try:
        out = []
        for nd in (False, True):
            st = {k: v.copy() for k, v in st0.items()}
            best = dict(seq=st["seqs"][0].copy(), ss=st["mfe_ss"][0].copy(),
                        vals=np.array([st["mcc1"][0], st["score"][0], st["Epf"][0], st["Ed"][0]] + ([0.0] if nd else [])))
            counters, rng = np.zeros(3, np.int64), hk.rng_seed(np.arange(R))
            sub = np.zeros(R)
            eng.mc_run(prob, 30, np.arange(R, dtype=np.int32), R, 0.7, 0.0, True, np.linspace(10, 150, R), [("Ed-Epf", 1.0)], flags, rng,
                       st, counters, best, **(dict(subopt_e=sub) if nd else {}))
            out.append((st, best, counters, rng, sub))
        (sa, ba, ca, ra, _), (sb, bb, cb, rb, sub) = out
        assert (sb["mcc1"] > 0).all() and bb["vals"][0] > 0 and not sub.any() and ca[0] > 0          # moved, never solved
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), k
        assert ba["seq"].tobytes() == bb["seq"].tobytes() and ba["ss"].tobytes() == bb["ss"].tobytes()
        assert ba["vals"].tobytes() == bb["vals"][:4].tobytes() and bb["vals"][4] == 0
        assert ca.tolist() == cb.tolist() and ra.tobytes() == rb.tobytes()
    finally:
        eng.close()


def test_null_subopt_e_is_an_argument_error(example_inputs):
    from desirna_amd import engine as E
    R = 2
    eng, prob, st = _mc_state(example_inputs, R)
    hk = E.HostKernels()
    try:
        E.HostKernels._pack(prob)
        am, partner, snake_of, off, nodes, nst, chars = prob._native_pack
        p = lambda a: a.ctypes.data
        ids, ws, sh, tt, cnt = np.zeros(1, np.int32), np.ones(1), np.zeros(R, np.int32), np.array([10.0, 20.0]), np.zeros(3, np.int64)
        bseq, bss, bv = st["seqs"][0].copy(), st["mfe_ss"][0].copy(), np.zeros(5)
        rc = eng._L.drna_mc_run_nd(eng._h, R, prob.n, 1, prob.sec_struct.encode(), p(partner), p(am), p(snake_of), 0, p(off), p(nodes),
                                   p(nst), p(chars), p(sh), R, 0.7, 0.0, 1, p(tt), 504.12, 1, p(ids), p(ws), 11,
                                   p(hk.rng_seed(np.arange(R))), p(st["seqs"]), p(st["mfe_ss"]), p(st["score"]), p(st["mcc1"]),
                                   p(st["Epf"]), p(st["Ed"]), p(cnt), p(bseq), p(bss), p(bv), None)
        assert rc == -1 and b"subopt_e" in eng._L.drna_last_error(eng._h)
        tg2 = example_inputs[HOM]["sec_struct"][0]
        cut = tg2.index("&")
        z = np.zeros(R)
        s2 = np.frombuffer((HOM_SOLVED * R).encode(), np.uint8).reshape(R, -1).copy()
        rc = eng._L.drna_mc_run_cofold_nd(eng._h, R, len(tg2) - 1, cut, 1, tg2.encode(), p(np.full(len(tg2), 15, np.uint8)), 2, p(sh), R,
                                          0.7, 0.0, 1, p(tt), 504.12, 1, p(ids), p(ws), p(hk.rng_seed(np.arange(R))), p(s2),
                                          p(s2.copy()), p(z), p(z), p(z), p(z), p(z), p(z), p(cnt), p(s2[0].copy()), p(s2[0].copy()),
                                          p(np.zeros(7)), None)
        assert rc == -1 and b"subopt_e" in eng._L.drna_last_error(eng._h)
    finally:
        eng.close()


def test_cli_nd_on_takes_the_native_driver_and_writes_the_python_drivers_subopt_e(example_inputs, tmp_path):
    inp = _inp(example_inputs, STD, STD_RESTR)
    f = tmp_path / "design.txt"
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (inp.name, inp.seq_restr, inp.sec_struct))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cols = []
    for extra in ([], ["--python-host"]):
        out = tmp_path / ("out" + str(len(extra)))
        res = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-R", "8", "-e", "10", "-s", "3", "-seed", "4",
                              "-nd", "on", "-o", str(out)] + extra, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert res.returncode == 0, res.stderr
        name = [n for n in os.listdir(out) if n.endswith("_results.csv")][0]
        rows = list(csv.DictReader(open(out / name)))
        assert rows and "subopt_e" in rows[0]
        cols.append([(r["sequence"], r["subopt_e"]) for r in rows])
    assert cols[0] == cols[1]
    assert any(float(e) != 0 for _, e in cols[0])
