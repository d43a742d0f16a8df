"""GPU box: device times of the auxiliary paths, one JSON line with a section per path (all, or those named as arguments).
Per shape the first round warms up and the median of the others is kept.
`sampling` (kept as profiles/sampling.json): the stochastic traceback at R = 64 x L = 200 x S = 1,024 next to the ensemble defect of
the same sequences, the other consumer of pf_kernel's tables.
`cofold_sampling` (kept as profiles/cofold_sampling.json): the two-strand stochastic traceback at 64 pairs of 18+18, 50+50 and
100+100 nt x S = 1,024 next to the two-strand ensemble defect of the same pairs and, at 100+100, the one-strand sampler on the
same letters read as single strands of 200.
`mea` (kept as profiles/mea.json): MEA and centroid structures (drna_mea_structures_batch) at R = 64 x L = 36, 100, 200, 400 and pairs
of 30+27 and 100+100: the inside, outside and MEA launches of the same call, the MEA launch with M in LDS and in the workspace
where the length allows both, and the candidates per column the pruning leaves.
`access` (only when named; kept as profiles/access.json): the partition function with positions held unpaired
(drna_pf_unpaired_batch) -- the masked general kernel beside the unmasked pf_kernel, the general kernel against the LDS kernel
over the lengths the latter holds, one accessibility profile of 1,930 folds, and what the design term costs per iteration.
`puzzle_set` (only when named; minutes): the Eterna100 set as a design run, lock-step batch against one puzzle after the other.
`puzzle_set_aux` (only when named): the same pair for the puzzles of at most 200 nt with -nd on, and with an Edef term added."""
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from desirna_amd import engine as E  # noqa: E402


def edef(eng, seqs):
    """ensemble defect (general inside kernel + outside kernel) at configs 3 and 5 shapes"""
    eng.ensemble_defect(seqs)
    t = eng.last_edef_timing()
    return {"inside_ms": t["inside"], "outside_ms": t["outside"]}


SAMPLES = 1024


def sampling(eng, seqs):
    """stochastic traceback (pf_kernel + sample_kernel, SAMPLES structures per sequence with their energies) and, in the same
    round, drna_ensemble_defect_batch on the same sequences (pf_kernel + outside_kernel)"""
    u8 = np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1)
    c0 = eng.get_option("sample_calls")
    eng.sample_structures_arrays(u8, SAMPLES, seed=1)
    t = eng.last_edef_timing()
    out = {"pf_ms": t["inside"], "sample_ms": t["outside"], "sample_launches": eng.get_option("sample_calls") - c0}
    eng.ensemble_defect(seqs)
    t = eng.last_edef_timing()
    out["edef_ms"] = t["inside"] + t["outside"]
    return out


def cofold_sampling(eng, seqs):
    """two-strand stochastic traceback (cofold_pf_kernel, then cofold_columns_kernel + cofold_sample_kernel, SAMPLES structures per
    pair with their energies); the same call with ONE sample per pair (its second figure is the columns launch plus an all but
    empty sample launch); drna_cofold_ensemble_defect_batch on the same pairs; at 100+100 also pf_kernel + sample_kernel on the
    same letters as single strands"""
    c0 = eng.get_option("cofold_sample_calls")
    eng.cofold_sample_structures(seqs, SAMPLES, seed=1)
    t = eng.last_edef_timing()
    out = {"cofold_pf_ms": t["inside"], "columns_and_sample_ms": t["outside"], "sample_launches": eng.get_option("cofold_sample_calls") - c0}
    eng.cofold_sample_structures(seqs, 1, seed=1)
    out["columns_and_one_sample_ms"] = eng.last_edef_timing()["outside"]
    eng.cofold_ensemble_defect(seqs)
    t = eng.last_edef_timing()
    out["cofold_edef_ms"] = t["inside"] + t["outside"]
    flat = [s.replace("&", "") for s in seqs]
    if len(flat[0]) == 200:
        u8 = np.frombuffer("".join(flat).encode(), dtype=np.uint8).reshape(len(flat), -1)
        eng.sample_structures_arrays(u8, SAMPLES, seed=1)
        t = eng.last_edef_timing()
        out["one_strand_pf_ms"], out["one_strand_sample_ms"] = t["inside"], t["outside"]
    return out


def mea(eng, seqs):
    """MEA and centroid structures with their energies at gamma = 1: the three launches of the call (short inputs: inside and
    outside are ONE fused launch, outside_ms ~ 0), the candidates per column that the pruning leaves, and, where M fits LDS, the MEA
    launch with M in the workspace instead"""
    two = "&" in seqs[0]
    call = eng.cofold_mea_structures if two else eng.mea_structures
    L = len(seqs[0].replace("&", ""))
    call(seqs, 1.0)
    t = eng.last_mea_timing()
    out = {"inside_ms": t["inside"], "outside_ms": t["outside"], "mea_ms": t["mea"],
           "candidates_per_column": eng.get_option("mea_candidates") / (len(seqs) * L)}
    if L <= eng.get_option("mea_lds_max"):
        eng.set_option("mea_lds", 0)
        call(seqs, 1.0)
        eng.set_option("mea_lds", 1)
        out["mea_ms_workspace"] = eng.last_mea_timing()["mea"]
    return out


def cofold_subopt(eng, seqs):
    """second-best co-fold kernel (two-strand -nd on) next to the co-fold MFE kernel"""
    eng.cofold_batch(seqs, E.NEED_MFE)
    m = eng.last_timing()["mfe"]
    eng.cofold_subopt_energy(seqs)
    return {"cofold_mfe_ms": m, "cofold_subopt_ms": eng.last_timing()["mfe"]}


def cofold_edef(eng, seqs):
    """two-strand outside kernel (-sf Edef) next to the co-fold partition function it runs after (a pair within
    cofold_edef_lds_max takes the fused launch: its time is the inside figure, the outside figure ~0)"""
    eng.cofold_batch(seqs, E.NEED_PF)
    p = eng.last_timing()["pf"]
    eng.cofold_ensemble_defect(seqs)
    t = eng.last_edef_timing()
    return {"cofold_pf_ms": p, "inside_in_edef_call_ms": t["inside"], "cofold_outside_ms": t["outside"]}


def subopt_energy(eng, seqs):
    """second-best structure energy (-nd on: every solved candidate of a scoring step), one strand or pairs, with the tables in
    LDS (option subopt_lds = 1) and on the general kernels (0), same process and engine; a sequence beyond subopt_lds_max
    takes the general kernels either way"""
    fn = eng.cofold_subopt_energy if "&" in seqs[0] else eng.subopt_energy
    out = {}
    for lds in (0, 1):
        eng.set_option("subopt_lds", lds)
        fn(seqs)
        out["subopt_ms_lds%d" % lds] = eng.last_timing()["mfe"]
    eng.set_option("subopt_lds", 1)
    return out


def subopt_structs(eng, seqs):
    """K lowest-energy structures with their strings (get_alt_mcc), both kernel instantiations"""
    out = {}
    for K in (4, 8):
        eng.subopt_structs(seqs, K)
        out["kbest%d_ms" % K] = eng.last_timing()["mfe"]
    return out


def cofold_kbest(eng, seqs):
    """K lowest-energy co-fold structures with their strings (get_alt_mcc of a two-strand design), both kernel instantiations,
    next to the one-strand kernel on the same letters read as single strands of the total length"""
    flat = [s.replace("&", "") for s in seqs]
    out = {}
    for K in (4, 8):
        eng.cofold_subopt_structs(seqs, K)
        out["cofold_kbest%d_ms" % K] = eng.last_timing()["mfe"]
        eng.subopt_structs(flat, K)
        out["kbest%d_ms" % K] = eng.last_timing()["mfe"]
    return out


def cofold_paths(eng, seqs):
    """both co-fold folds with the tables in LDS (option cofold_lds = 1) and on the general kernels (0), same process and engine;
    a pair beyond the bound takes the general kernels either way"""
    out = {}
    for lds in (0, 1):
        eng.set_option("cofold_lds", lds)
        eng.cofold_batch(seqs, E.NEED_MFE | E.NEED_PF)
        t = eng.last_timing()
        out["mfe_ms_lds%d" % lds], out["pf_ms_lds%d" % lds] = t["mfe"], t["pf"]
    eng.set_option("cofold_lds", 1)
    return out


def self_dimer(eng, seqs):
    """every sequence against a copy of itself (-oa on) with the tables in LDS (option self_dimer_lds = 1) and in the workspace
    slots (0), same process and engine; a sequence beyond self_dimer_lds_max takes the workspace kernel either way"""
    out = {}
    for lds in (0, 1):
        eng.set_option("self_dimer_lds", lds)
        eng.self_dimer(seqs)
        out["pf_ms_lds%d" % lds] = eng.last_timing()["pf"]
    eng.set_option("self_dimer_lds", 1)
    return out


MC_TARGET = "((((((..((((......&......))))..))))))"       # 18 + 18 nt
MC_RESTR = "N" * 18 + "&" + "N" * 18
MC_ITERS = 200


def mc_cofold(eng, seqs):
    """wall time per iteration of drna_mc_run_cofold (64 replicas of 18 + 18 nt, -sf Ed-Epf, targeted moves on), and the same
    design (same seed, 2 exchange steps of 20 iterations) through run_design_fast's native loop and through run_design"""
    from desirna_amd import design
    R = len(seqs)
    prob = design.DesignProblem(MC_TARGET, MC_RESTR)
    hk = E.HostKernels()
    eng.set_targets([MC_TARGET.replace("&", "")])
    cur = np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(R, -1).copy()
    co = eng.cofold_batch(seqs)
    state = dict(seqs=cur, mfe_ss=np.frombuffer("".join(co["mfe_ss"]).encode(), dtype=np.uint8).reshape(R, -1).copy(),
                 score=np.full(R, 1e3), mcc1=np.ones(R), Epf=np.zeros(R), Ed=np.zeros(R), oligo_fraction=np.zeros(R), bonus=np.zeros(R))
    best = dict(seq=cur[0].copy(), ss=state["mfe_ss"][0].copy(), vals=np.array([1.0, 1e3, 0, 0, 0, 0]))
    rng_state = hk.rng_seed(np.arange(R))
    temps = np.linspace(10.0, 150.0, R)
    t0 = time.perf_counter()
    eng.mc_run_cofold(prob, "heterodimer", MC_ITERS, np.arange(R, dtype=np.int32), R, 0.7, 0.0, True, temps, [("Ed-Epf", 1.0)],
                      rng_state, state, np.zeros(3, dtype=np.int64), best)
    out = {"mc_iter_wall_ms": (time.perf_counter() - t0) * 1e3 / MC_ITERS}
    inp = SimpleNamespace(name="pair", sec_struct=MC_TARGET, seq_restr=MC_RESTR, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    kw = dict(replicas=R, exchange=20, steps=2, seed=3, timelimit=600)
    for key, run in (("native", lambda: design.run_design_fast(inp, engine=eng, **kw)), ("python", lambda: design.run_design(inp, **kw))):
        t0 = time.perf_counter()
        res = run()
        out["design_%s_iter_per_s" % key] = res["steps"] * 20 / (time.perf_counter() - t0)
    return out


ND_TARGET = "((((((.((((((((....))))).)).).))))))"                # the reference's 36-nt example
ND_RESTR = "GCCCCGGCCCCCGGCNNNNGCCGGUGGNGGCGGGGC"                 # initial sequence = a solved one: every iteration folds second-best structures


def nd_loop(eng, seqs):
    """scored sequences per second of a -nd on design (64 replicas x 36 nt from a solved start, 3 exchange steps of 50
    iterations) through the native loop (drna_mc_run_nd) and through the per-iteration loop"""
    from desirna_amd import design
    R = len(seqs)
    inp = SimpleNamespace(name="nd", sec_struct=ND_TARGET, seq_restr=ND_RESTR, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    kw = dict(replicas=R, exchange=50, steps=3, seed=3, timelimit=600, negative_design="on", engine=eng, keep_records=False)
    out = {}
    for key, native in (("native", True), ("per_iteration", False)):
        t0 = time.perf_counter()
        res = design.run_design_fast(inp, native_loop=native, **kw)
        out["nd_%s_scored_per_s" % key] = res["stats"]["scored"] / (time.perf_counter() - t0)
    return out


def edef_paths(eng, seqs):
    """ensemble defect (-sf Edef) through the fused LDS kernel (option edef_lds = 1: one launch) and through the general inside +
    outside kernels (0), same process and engine; at the reference's design sizes (36 nt, 18 + 18 nt) also the wall time per
    iteration of the native Monte-Carlo loop with -sf Edef:1.0 (2 exchange steps of 20 iterations, same seed) either way"""
    from desirna_amd import design
    two = "&" in seqs[0]
    R, L = len(seqs), len(seqs[0].replace("&", ""))
    fn = eng.cofold_ensemble_defect if two else eng.ensemble_defect
    loop = L == 36
    inp = SimpleNamespace(name="edef", sec_struct=MC_TARGET if two else ND_TARGET, seq_restr=MC_RESTR if two else "N" * 36,
                          seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)
    out = {}
    for lds in (0, 1):
        eng.set_option("edef_lds", lds)
        eng.set_targets(["." * L])
        c0 = eng.get_option("edef_lds_calls")
        fn(seqs)
        t = eng.last_edef_timing()
        out["edef_ms_lds%d" % lds] = t["inside"] + t["outside"]
        out["fused_launches_lds%d" % lds] = eng.get_option("edef_lds_calls") - c0
        if loop:
            t0 = time.perf_counter()
            res = design.run_design_fast(inp, engine=eng, replicas=R, exchange=20, steps=2, seed=3, timelimit=600, scoring_f="Edef:1.0",
                                         keep_records=False)
            out["mc_iter_wall_ms_lds%d" % lds] = (time.perf_counter() - t0) * 1e3 / (res["steps"] * 20)
    eng.set_option("edef_lds", 1)
    return out


PAIRS = ((64, 18, 18), (64, 50, 50), (64, 100, 100))
SUB_MAX = 79          # SUB_LDS_MAX (fold_subopt_lds.hpp)
CO_HALF = 32          # CO_LDS_MAX / 2 (fold_cofold_lds.hpp)
SD_MAX = 62           # SD_LDS_MAX (fold_self_dimer.hpp)
EDEF_MAX = 40         # EDEF_LDS_HOST_MAX (fold_edef_lds.hpp)
CO_EDEF_MAX = 57      # CO_EDEF_LDS_MAX
# one round of a section -> (shapes (R, strand lengths ...), seed, a fresh generator per shape, rounds, derived figure)
SECTIONS = {
    edef: (((64, 200), (128, 400)), 20260101, True, 3,
           lambda R, v: ("defects_per_s", R / ((v["inside_ms"] + v["outside_ms"]) * 1e-3))),
    sampling: (((64, 200),), 20260101, True, 5,
               lambda R, v: ("samples_per_s", R * SAMPLES / (v["sample_ms"] * 1e-3))),
    cofold_sampling: (PAIRS, 5, False, 5,
                      lambda R, v: ("samples_per_s", R * SAMPLES / (v["columns_and_sample_ms"] * 1e-3))),
    cofold_subopt: (PAIRS, 5, False, 5, lambda R, v: ("ratio", v["cofold_subopt_ms"] / v["cofold_mfe_ms"])),
    cofold_edef: (PAIRS, 5, False, 5, lambda R, v: ("ratio", v["cofold_outside_ms"] / v["cofold_pf_ms"])),
    subopt_energy: (((64, 36), (64, SUB_MAX), (64, 18, 18), (64, 100), (64, 200)), 5, False, 5,
                    lambda R, v: ("lds_over_general", v["subopt_ms_lds1"] / v["subopt_ms_lds0"])),
    nd_loop: (((64, 36),), 5, False, 3,
              lambda R, v: ("native_over_per_iteration", v["nd_native_scored_per_s"] / v["nd_per_iteration_scored_per_s"])),
    subopt_structs: (((16, 100), (16, 200)), 5, False, 5, lambda R, v: ("ratio", v["kbest8_ms"] / v["kbest4_ms"])),
    cofold_kbest: (((16, 18, 18), (16, 50, 50)), 5, False, 5,
                   lambda R, v: ("ratio_k8", v["cofold_kbest8_ms"] / v["kbest8_ms"])),
    cofold_paths: (((64, 18, 18), (64, CO_HALF, CO_HALF), (64, CO_HALF + 1, CO_HALF)), 5, False, 7,
                   lambda R, v: ("lds_over_general", (v["mfe_ms_lds1"] + v["pf_ms_lds1"]) / (v["mfe_ms_lds0"] + v["pf_ms_lds0"]))),
    self_dimer: (((64, 36), (64, SD_MAX), (64, 100)), 5, False, 7, lambda R, v: ("lds_over_general", v["pf_ms_lds1"] / v["pf_ms_lds0"])),
    edef_paths: (((64, 36), (64, 18, 18), (64, EDEF_MAX), (64, CO_EDEF_MAX // 2, CO_EDEF_MAX - CO_EDEF_MAX // 2)), 5, False, 5,
                 lambda R, v: ("lds_over_general", v["edef_ms_lds1"] / v["edef_ms_lds0"])),
    mea: (((64, 36), (64, 100), (64, 200), (64, 400), (64, 30, 27), (64, 100, 100)), 5, False, 5,
          lambda R, v: ("mea_over_inside_outside", v["mea_ms"] / (v["inside_ms"] + v["outside_ms"]))),
    mc_cofold: (((64, 18, 18),), 5, False, 3,
                lambda R, v: ("native_over_python", v["design_native_iter_per_s"] / v["design_python_iter_per_s"])),
}


def section_inputs(name):
    """(key, R, total length, sequences) of every shape of a section, as the timing loop below draws them"""
    one_round = next(f for f in SECTIONS if f.__name__ == name)
    shapes, seed, reseed = SECTIONS[one_round][:3]
    rng = np.random.default_rng(seed)
    for R, *lens in shapes:
        rng = np.random.default_rng(seed) if reseed else rng
        seqs = ["&".join("".join(rng.choice(list("ACGU"), n)) for n in lens) for _ in range(R)]
        yield "R%d_" % R + ("L%d" % lens[0] if len(lens) == 1 else "%d+%d" % tuple(lens)), R, sum(lens), seqs


PS_REPLICAS, PS_EXCHANGE, PS_STEPS, PS_SEED = 32, 10, 5, 5          # one warm-up exchange step + four timed ones


def _step_times(eng, method, run):
    """wall seconds of every exchange step of run(): from one call of the engine's native loop `method` to the next (so the
    step's Python work -- ladder, exchange, records -- counts), the last one to the end of the run"""
    starts, inner = [], getattr(eng, method)

    def timed(*a, **kw):
        starts.append(time.perf_counter())
        return inner(*a, **kw)

    setattr(eng, method, timed)
    try:
        run()
    finally:
        delattr(eng, method)
    starts.append(time.perf_counter())
    return np.diff(starts)


def _puzzle_inputs():
    import csv
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "eterna_v1_targets.csv")
    return [SimpleNamespace(name=r["name"], sec_struct=r["structure"], seq_restr="N" * len(r["structure"]), seed_seq=None,
                            alt_sec_struct=None, alt_sec_structs=None) for r in csv.DictReader(open(path))]


def _lockstep(inputs, method="mc_run_ragged", **switches):
    """median wall ms of an exchange step of run_puzzle_batch over `inputs` (the first step warms up)"""
    from desirna_amd import design
    eng = E.Engine(max_R=len(inputs) * PS_REPLICAS, max_L=max(len(i.sec_struct) for i in inputs), device=0)
    kw = dict(replicas=PS_REPLICAS, exchange=PS_EXCHANGE, steps=PS_STEPS, seed=PS_SEED, timelimit=36000, engine=eng, **switches)
    d = _step_times(eng, method, lambda: design.run_puzzle_batch(inputs, **kw))
    eng.close()
    assert len(d) == PS_STEPS
    return float(np.median(d[1:])) * 1e3


def puzzle_set():
    """BASELINE config 4 as a design run: the 100 Eterna100 targets x 32 replicas, exchange = 10, fixed seed.  (a) lock-step,
    run_puzzle_batch; (b) today's path, run_design_fast one puzzle after the other on an engine of the puzzle's size, summed.
    Same process, same visit; the same pair for the puzzles of at most 200 nt.  The host split of the lock-step run comes from
    a child process with DRNA_MC_PROFILE set (its stderr lines, averaged over the calls after the first)."""
    import re
    import subprocess
    from desirna_amd import design
    inputs = _puzzle_inputs()
    short = [i for i in inputs if len(i.sec_struct) <= 200]
    per = {}
    for inp in inputs:
        eng = E.Engine(max_R=PS_REPLICAS, max_L=len(inp.sec_struct), device=0)
        kw = dict(replicas=PS_REPLICAS, exchange=PS_EXCHANGE, steps=PS_STEPS, seed=PS_SEED, timelimit=36000, engine=eng)
        d = _step_times(eng, "mc_run", lambda: design.run_design_fast(inp, **kw))
        eng.close()
        assert len(d) == PS_STEPS
        per[inp.name] = float(np.median(d[1:])) * 1e3
    out = {}
    for key, sub in (("all", inputs), ("le200", short)):
        lock, one_by_one = _lockstep(sub), sum(per[i.name] for i in sub)
        chains = len(sub) * PS_REPLICAS
        out[key] = {"puzzles": len(sub), "chains": chains, "lockstep_step_ms": lock, "per_puzzle_sum_step_ms": one_by_one,
                    "lockstep_over_per_puzzle": lock / one_by_one,
                    "lockstep_chain_iters_per_s": chains * PS_EXCHANGE / (lock * 1e-3),
                    "per_puzzle_chain_iters_per_s": chains * PS_EXCHANGE / (one_by_one * 1e-3)}
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "puzzle_set_profile"], env=dict(os.environ, DRNA_MC_PROFILE="1"),
                           stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, check=True)
    rows = re.findall(r"drna_mc_run_ragged: per iteration, host us: score call beyond device time ([-0-9.]+), per-replica work ([-0-9.]+), "
                      r"bookkeeping ([-0-9.]+)", child.stderr)
    rows = np.array(rows[1:], dtype=np.float64)
    out["all"]["host_us_per_iteration"] = dict(zip(("score_call_beyond_device", "per_chain_work", "bookkeeping"),
                                                   (float(x) for x in np.median(rows, axis=0))))
    return out


AUX_SWITCHES = (("nd", dict(negative_design="on")), ("nd_edef", dict(negative_design="on", scoring_f="Ed-Epf:1.0,Edef:1.0")))


def puzzle_set_aux():
    """The 71 Eterna100 targets of at most 200 nt x 32 replicas, exchange = 10, fixed seed, with -nd on and then with Edef:1.0
    added to the scoring function: (a) lock-step, run_puzzle_batch on drna_mc_run_ragged_nd; (b) run_design_fast one puzzle after
    the other on an engine of the puzzle's size, summed.  Same process, same visit, medians after a warm-up step."""
    from desirna_amd import design
    from desirna_amd import energy_scores as es
    keep_first = es.parse_scoring_functions
    es.parse_scoring_functions = lambda s, first_term_only=True: keep_first(s, False)     # (the reference keeps the first -sf term only)
    inputs = [i for i in _puzzle_inputs() if len(i.sec_struct) <= 200]
    out = {}
    for key, switches in AUX_SWITCHES:
        one_by_one = 0.0
        for inp in inputs:
            eng = E.Engine(max_R=PS_REPLICAS, max_L=len(inp.sec_struct), device=0)
            kw = dict(replicas=PS_REPLICAS, exchange=PS_EXCHANGE, steps=PS_STEPS, seed=PS_SEED, timelimit=36000, engine=eng, **switches)
            d = _step_times(eng, "mc_run", lambda: design.run_design_fast(inp, **kw))
            eng.close()
            assert len(d) == PS_STEPS
            one_by_one += float(np.median(d[1:])) * 1e3
        lock = _lockstep(inputs, "mc_run_ragged_nd", **switches)
        chains = len(inputs) * PS_REPLICAS
        out[key] = {"puzzles": len(inputs), "chains": chains, "lockstep_step_ms": lock, "per_puzzle_sum_step_ms": one_by_one,
                    "lockstep_over_per_puzzle": lock / one_by_one,
                    "lockstep_chain_iters_per_s": chains * PS_EXCHANGE / (lock * 1e-3),
                    "per_puzzle_chain_iters_per_s": chains * PS_EXCHANGE / (one_by_one * 1e-3)}
    es.parse_scoring_functions = keep_first
    return out


ACCESS_ROUNDS = 9            # per figure: one warm-up round, then the median, lowest and highest of the others
ACCESS_TARGETS = {36: ND_TARGET, 200: "." * 20 + ND_TARGET + "." * 30 + "((((((((....))))))))" + "." * 38 + ND_TARGET + "." * 20}


def _spread(values):
    v = np.array(values[1:], dtype=np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def access():
    """Device times (events; drna_last_access_timing) of drna_pf_unpaired_batch at R = 64, M = 1, random ACGU sequences, a random
    mask of 8 positions, the paths alternating round by round in one process:
      general_vs_unmasked   pf_kernel<1024, true> (option access_lds = 0) beside the unmasked pf_kernel<1024> (the inside launch of
                            drna_ensemble_defect_batch with edef_lds = 0) at 36, 100, 200 and 400 nt
      lds_vs_general        access_lds_kernel (option access_lds = 2: whatever the host's bound) against pf_kernel<1024, true> at
                            24, 36, 48, 64, 80 nt and the kernel's bound: the table that fixes ACCESS_LDS_HOST_MAX
      profile               ONE call of 10 sequences x 200 nt x every window of 8 (1,930 folds) on an engine of 64 slots
      design_term           run_design_fast(native_loop=False), 64 replicas x 36 and 200 nt: wall ms per iteration with and without
                            an >accessible region of 8 nt, and the device ms of the fused launch that gives Epf beside the masked fill"""
    from desirna_amd import design
    rng = np.random.default_rng(20261)
    R = 64
    out = {"general_vs_unmasked": {}, "lds_vs_general": {}, "design_term": {}}

    def shape(L, lds_too, plain_too):
        seqs = ["".join(rng.choice(list("ACGU"), L)) for _ in range(R)]
        mask = np.zeros((1, L), dtype=np.uint8)
        mask[0, rng.choice(L, 8, replace=False)] = 1
        eng = E.Engine(max_R=R, max_L=L, device=0)
        eng.set_targets(["." * L])
        eng.set_option("edef_lds", 0)
        t = {"general": [], "lds": [], "unmasked": []}
        for _ in range(ACCESS_ROUNDS):
            eng.set_option("access_lds", 0)
            eng.unpaired_free_energy(seqs, mask)
            t["general"].append(eng.last_access_timing())
            if lds_too:
                eng.set_option("access_lds", 2)            # (2: beyond the host's bound, up to the kernel's)
                c0 = eng.get_option("access_lds_calls")
                eng.unpaired_free_energy(seqs, mask)
                assert eng.get_option("access_lds_calls") == c0 + 1
                t["lds"].append(eng.last_access_timing())
            if plain_too:
                eng.ensemble_defect(seqs)
                t["unmasked"].append(eng.last_edef_timing()["inside"])
        eng.close()
        return {k: _spread(v) for k, v in t.items() if v}

    for L in (36, 100, 200, 400):
        out["general_vs_unmasked"]["R%d_L%d" % (R, L)] = shape(L, False, True)
    eng = E.Engine(max_R=1, max_L=8, device=0)
    out["access_lds_max_option"], kernel_max = eng.get_option("access_lds_max"), eng.get_option("access_lds_kernel_max")
    eng.close()
    for L in sorted({24, 36, 48, 64, 80, kernel_max}):
        out["lds_vs_general"]["R%d_L%d" % (R, L)] = shape(L, True, False)
    # one accessibility profile
    L, W, n_seq = 200, 8, 10
    seqs = ["".join(rng.choice(list("ACGU"), L)) for _ in range(n_seq)]
    masks = np.zeros((L - W + 1, L), dtype=np.uint8)
    for a in range(L - W + 1):
        masks[a, a:a + W] = 1
    eng = E.Engine(max_R=R, max_L=L, device=0)
    ms, wall = [], []
    for _ in range(4):
        t0 = time.perf_counter()
        eng.unpaired_free_energy(seqs, masks)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(eng.last_access_timing())
    slots = eng.get_option("workspace_slots")
    folds = n_seq * masks.shape[0]
    out["profile"] = {"folds": folds, "workspace_slots": slots, "chunks": -(-folds // slots), "device": _spread(ms), "wall": _spread(wall)}
    eng.close()
    # the term inside a design
    for L, target in ACCESS_TARGETS.items():
        assert len(target) == L
        free = target.index("....") if L == 36 else 0
        region = "." * free + "x" * 8 + "." * (L - free - 8)
        eng = E.Engine(max_R=R, max_L=L, device=0)
        v = {}
        for key, acc in (("plain", None), ("region", region), ("plain_again", None)):
            inp = SimpleNamespace(name="acc", sec_struct=target, seq_restr="N" * L, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None,
                                  accessible=acc)
            t0 = time.perf_counter()
            res = design.run_design_fast(inp, engine=eng, replicas=R, exchange=20, steps=3, seed=3, timelimit=600, native_loop=False,
                                         keep_records=False)
            v["iter_wall_ms_" + key] = (time.perf_counter() - t0) * 1e3 / (res["steps"] * 20 + 1)
        seqs = ["".join(rng.choice(list("ACGU"), L)) for _ in range(R)]
        fused, masked = [], []
        for _ in range(ACCESS_ROUNDS):
            eng.score_batch(seqs)
            fused.append(eng.last_timing()["total"])
            eng.unpaired_free_energy(seqs, region)
            masked.append(eng.last_access_timing())
        v["score_batch_device"], v["masked_fill_device"] = _spread(fused), _spread(masked)
        v["masked_over_score_batch"] = v["masked_fill_device"]["median_ms"] / v["score_batch_device"]["median_ms"]
        out["design_term"]["R%d_L%d" % (R, L)] = v
        eng.close()
    return out


def main(names):
    if names == ["puzzle_set_profile"]:                      # the child of puzzle_set: the lock-step run alone, profile lines on stderr
        _lockstep(_puzzle_inputs())
        return
    out = {}
    whole_runs = {"puzzle_set": puzzle_set, "puzzle_set_aux": puzzle_set_aux, "access": access}
    if set(names) & set(whole_runs):
        for n in names:
            if n in whole_runs:
                out[n] = whole_runs[n]()
        names = [n for n in names if n not in whole_runs]
        if not names:
            print(json.dumps(out))
            return
    for one_round, (_, _, _, rounds, derived) in SECTIONS.items():
        if names and one_round.__name__ not in names:
            continue
        sec = out[one_round.__name__] = {}
        for key, R, L, seqs in section_inputs(one_round.__name__):
            eng = E.Engine(max_R=R, max_L=L, device=0)
            eng.set_targets(["." * L])
            runs = [one_round(eng, seqs) for _ in range(rounds)]
            v = {k: float(np.median([r[k] for r in runs[1:]])) for k in runs[0]}
            v.update([derived(R, v)])
            sec[key] = v
            eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
