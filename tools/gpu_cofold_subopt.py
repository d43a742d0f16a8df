"""GPU box: device time of the second-best co-fold kernel (two-strand -nd on) next to the co-fold MFE kernel."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from desirna_amd import engine as E
out = {}
rng = np.random.default_rng(5)
for R, la, lb in ((64, 18, 18), (64, 50, 50), (64, 100, 100)):
    seqs = ["".join(rng.choice(list("ACGU"), la)) + "&" + "".join(rng.choice(list("ACGU"), lb)) for _ in range(R)]
    eng = E.Engine(max_R=R, max_L=la + lb, device=0)
    mfe, sub = [], []
    for _ in range(5):                                   # the first round warms up; the median of the other four is kept
        eng.cofold_batch(seqs, E.NEED_MFE)
        mfe.append(eng.last_timing()["mfe"])
        eng.cofold_subopt_energy(seqs)
        sub.append(eng.last_timing()["mfe"])
    m, s = float(np.median(mfe[1:])), float(np.median(sub[1:]))
    out["R%d_%d+%d" % (R, la, lb)] = {"cofold_mfe_ms": m, "cofold_subopt_ms": s, "ratio": s / m}
    eng.close()
print(json.dumps(out))
