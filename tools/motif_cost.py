"""GPU box: what the motif term (-motifs) costs the native Monte-Carlo loop, one JSON document (profiles/motifs.json).

Wall time per iteration of drna_mc_run over 300 iterations (after one untimed call of 300), median of five repeats, at
R = 64 x L = 200 (eteV1_69) and R = 64 x L = 36 (eteV1_03), -sf Ed-Epf:1.0, targeted moves on; the run's own device and host time
per iteration from drna_timing_sums.  Every figure comes from a process of its own, one after the other:

    parent, this tree, parent, this tree      with no motifs  (`--parent-lib`: the library built from the parent commit)
    this tree                                 with 1 and with 4 motifs of 4 .. 8 letters

    python tools/motif_cost.py --parent-lib /path/to/parent/libdesirna_amd.so > profiles/motifs.json

Condition: with no motifs this tree lies within the parent's own spread, the distance between the parent's two processes (the
margin of DESIGN 3.5a).  The cost per motif is reported, not bounded."""
import argparse
import ctypes
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("R64_L200", 64, "eteV1_69.txt"), ("R64_L36", 64, "eteV1_03.txt"))
ITERS, REPEATS = 300, 5
MOTIF_SETS = {0: "", 1: "GNRA,-2", 4: "GNRA,-2,GGGG,3,UUCGNNYR,-1,CWSAAG,1.5"}          # 4, 4, 8 and 6 letters


def _target(name):
    import csv
    with open(os.path.join(ROOT, "tests", "golden", "eterna_v1_targets.csv")) as fh:
        return next(r["structure"] for r in csv.DictReader(fh) if r["name"] == name)


def child(lib, n_motifs):
    """one process: both shapes on the library `lib` with MOTIF_SETS[n_motifs]"""
    from desirna_amd import design, engine as E, replica_exchange as rx
    from desirna_amd import energy_scores as es
    have = ctypes.CDLL(lib)
    for name in [n for n in E._SIGNATURES if not hasattr(have, n)]:          # (a parent build has no motif symbols)
        del E._SIGNATURES[name]
    assert n_motifs == 0 or "drna_set_motifs" in E._SIGNATURES
    out = {}
    for key, R, name in SHAPES:
        target = _target(name)
        L = len(target)
        eng = E.Engine(max_R=R, max_L=L, lib=lib)
        hk = E.HostKernels(lib)
        eng.set_targets([target])
        if n_motifs:
            eng.set_motifs(es.parse_motifs(MOTIF_SETS[n_motifs]))
            assert eng.get_option("motifs") == n_motifs
        prob = design.DesignProblem(target, "N" * L, None)
        flags, sf = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL, [("Ed-Epf", 1.0)]
        init = prob.initial_sequence(random.Random(2138))
        cur = np.ascontiguousarray(np.tile(np.frombuffer(init.encode(), dtype=np.uint8), (R, 1)))
        Epf, _, ss, Ed = eng.score_batch_arrays(cur, flags)
        mcc, _, _ = hk.simscore(target, ss)
        state = dict(seqs=cur, mfe_ss=np.ascontiguousarray(ss), score=np.ascontiguousarray(Ed[:, 0] / 100.0 - Epf),
                     mcc1=np.ascontiguousarray(1.0 - mcc), Epf=np.ascontiguousarray(Epf), Ed=np.ascontiguousarray(Ed[:, 0] / 100.0))
        temps = np.array(rx.get_rep_temps(R, 10.0, 150.0), dtype=np.float64)
        shelf = np.searchsorted(temps, temps).astype(np.int32)
        rng_state = np.empty((R, E.RNG_WORDS), dtype=np.uint32)
        counters = np.zeros(3, dtype=np.int64)
        best = dict(seq=cur[0].copy(), ss=state["mfe_ss"][0].copy(),
                    vals=np.array([state["mcc1"][0], state["score"][0], state["Epf"][0], state["Ed"][0]], dtype=np.float64))
        wall, dev = [], []
        for rep in range(REPEATS + 1):                          # the first call warms up (and the replicas diverge)
            hk.rng_seed(np.arange(R), out=rng_state)
            eng.timing_sums(reset=True)
            t0 = time.perf_counter()
            eng.mc_run(prob, ITERS, shelf, R, 0.7, 0.0, True, temps, sf, flags, rng_state, state, counters, best)
            dt = time.perf_counter() - t0
            ts = eng.timing_sums()
            if rep:
                wall.append(dt / ITERS * 1e6)
                dev.append(ts["total"] / max(1, ts["calls"]) * 1e3)
        w, d = float(np.median(wall)), float(np.median(dev))
        out[key] = {"wall_us_per_iteration": w, "device_us_per_iteration": d, "host_us_per_iteration": w - d,
                    "wall_us_repeats": [round(x, 2) for x in wall], "accepted": int(counters[0]), "rejected": int(counters[2])}
        eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libdesirna_amd.so built from the parent commit")
    ap.add_argument("--child", nargs=2, metavar=("LIB", "N_MOTIFS"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    from desirna_amd import engine as E
    new = E.LIB_PATH

    def run(lib, n):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(n)], stdout=subprocess.PIPE, text=True,
                             check=True, timeout=600)
        return json.loads(res.stdout.strip().splitlines()[-1])

    order = ([("parent", a.parent_lib)] if a.parent_lib else []) + [("new", new)]
    procs = {"parent": [], "new": []}
    for _ in range(2):
        for who, lib in order:
            procs[who].append(run(lib, 0))
    with_motifs = {n: run(new, n) for n in (1, 4)}
    out = {"what": __doc__.split("\n\n")[1].replace("\n", " "), "iterations": ITERS, "repeats": REPEATS,
           "motif_sets": {str(n): MOTIF_SETS[n] for n in (1, 4)}, "shapes": {}}
    for key, R, name in SHAPES:
        w = lambda rows: [r[key]["wall_us_per_iteration"] for r in rows]
        s = out["shapes"][key] = {"target": name, "no_motifs_new": [r[key] for r in procs["new"]],
                                  "no_motifs_parent": [r[key] for r in procs["parent"]]}
        new0 = float(np.mean(w(procs["new"])))
        if a.parent_lib:
            p = w(procs["parent"])
            s["parent_spread_us"] = abs(p[0] - p[1])
            s["new_minus_parent_us"] = new0 - float(np.mean(p))
            s["within_parent_spread"] = bool(abs(s["new_minus_parent_us"]) <= s["parent_spread_us"])
        host0 = float(np.mean([r[key]["host_us_per_iteration"] for r in procs["new"]]))
        s["host_us_per_iteration_no_motifs"] = host0
        for n, r in with_motifs.items():
            s["motifs_%d" % n] = r[key]
            s["motifs_%d_added_us" % n] = r[key]["wall_us_per_iteration"] - new0
            s["motifs_%d_added_host_us" % n] = r[key]["host_us_per_iteration"] - host0          # (the walk, so the device time, differs too)
        s["four_motifs_exceed_the_runs_host_time"] = bool(s["motifs_4_added_us"] > host0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
