"""GPU box: device times of the auxiliary paths, one JSON line with a section per path (all, or those named as arguments).
Per shape the first round warms up and the median of the others is kept."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from desirna_amd import engine as E  # noqa: E402


def edef(eng, seqs):
    """ensemble defect (general inside kernel + outside kernel) at configs 3 and 5 shapes"""
    eng.ensemble_defect(seqs)
    t = eng.last_edef_timing()
    return {"inside_ms": t["inside"], "outside_ms": t["outside"]}


def cofold_subopt(eng, seqs):
    """second-best co-fold kernel (two-strand -nd on) next to the co-fold MFE kernel"""
    eng.cofold_batch(seqs, E.NEED_MFE)
    m = eng.last_timing()["mfe"]
    eng.cofold_subopt_energy(seqs)
    return {"cofold_mfe_ms": m, "cofold_subopt_ms": eng.last_timing()["mfe"]}


def cofold_edef(eng, seqs):
    """two-strand outside kernel (-sf Edef) next to the co-fold partition function it runs after"""
    eng.cofold_batch(seqs, E.NEED_PF)
    p = eng.last_timing()["pf"]
    eng.cofold_ensemble_defect(seqs)
    t = eng.last_edef_timing()
    return {"cofold_pf_ms": p, "inside_in_edef_call_ms": t["inside"], "cofold_outside_ms": t["outside"]}


def subopt_energy(eng, seqs):
    """second-best structure energy of one strand (-nd on, every scoring step)"""
    eng.subopt_energy(seqs)
    return {"subopt_ms": eng.last_timing()["mfe"]}


def subopt_structs(eng, seqs):
    """K lowest-energy structures with their strings (get_alt_mcc), both kernel instantiations"""
    out = {}
    for K in (4, 8):
        eng.subopt_structs(seqs, K)
        out["kbest%d_ms" % K] = eng.last_timing()["mfe"]
    return out


PAIRS = ((64, 18, 18), (64, 50, 50), (64, 100, 100))
# one round of a section -> (shapes (R, strand lengths ...), seed, a fresh generator per shape, rounds, derived figure)
SECTIONS = {
    edef: (((64, 200), (128, 400)), 20260101, True, 3,
           lambda R, v: ("defects_per_s", R / ((v["inside_ms"] + v["outside_ms"]) * 1e-3))),
    cofold_subopt: (PAIRS, 5, False, 5, lambda R, v: ("ratio", v["cofold_subopt_ms"] / v["cofold_mfe_ms"])),
    cofold_edef: (PAIRS, 5, False, 5, lambda R, v: ("ratio", v["cofold_outside_ms"] / v["cofold_pf_ms"])),
    subopt_energy: (((64, 36), (64, 100), (64, 200)), 5, False, 5, lambda R, v: ("folds_per_s", R / (v["subopt_ms"] * 1e-3))),
    subopt_structs: (((16, 100), (16, 200)), 5, False, 5, lambda R, v: ("ratio", v["kbest8_ms"] / v["kbest4_ms"])),
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


def main(names):
    out = {}
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
