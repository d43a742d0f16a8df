"""GPU box: device time of the two-strand outside kernel (-sf Edef) next to the co-fold partition function it runs after."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from desirna_amd import engine as E
out = {}
rng = np.random.default_rng(5)
for R, la, lb in ((64, 18, 18), (64, 50, 50), (64, 100, 100)):
    seqs = ["".join(rng.choice(list("ACGU"), la)) + "&" + "".join(rng.choice(list("ACGU"), lb)) for _ in range(R)]
    eng = E.Engine(max_R=R, max_L=la + lb, device=0)
    eng.set_targets(["." * (la + lb)])
    pf, ins, outs = [], [], []
    for _ in range(5):                                   # the first round warms up; the median of the other four is kept
        eng.cofold_batch(seqs, E.NEED_PF)
        pf.append(eng.last_timing()["pf"])
        eng.cofold_ensemble_defect(seqs)
        t = eng.last_edef_timing()
        ins.append(t["inside"]); outs.append(t["outside"])
    p, i, o = (float(np.median(x[1:])) for x in (pf, ins, outs))
    out["R%d_%d+%d" % (R, la, lb)] = {"cofold_pf_ms": p, "inside_in_edef_call_ms": i, "cofold_outside_ms": o, "ratio": o / p}
    eng.close()
print(json.dumps(out))
