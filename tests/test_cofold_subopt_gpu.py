"""Second-best co-fold energy on the GPU (drna_cofold_subopt_energy_batch, cofold_subopt_kernel): two-strand -nd on.

The reference pins no subopt output for two strands; the GPU is checked bit for bit against the CPU emulation of the same
kernel source (which tests/test_cofold_subopt_emulated.py checks against exhaustive enumeration), against the oracle's co-fold
MFE and the golden mfe_dimer structures, and against properties of the structure set at lengths the emulation cannot reach."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests.emu.emu import INF_REF, cofold_subopt_many

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=128, max_L=400, device=0)
    yield e
    e.close()


def _rand(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def _e2(e12):
    return e12[1] if e12[1] < INF_REF and e12[1] - e12[0] <= 4900 else 0


def _rotate(db, cut):
    n = len(db)
    stack, out = [], ["."] * n
    for k, ch in enumerate(db):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            a, b = sorted(((stack.pop() + cut) % n, (k + cut) % n))
            out[a], out[b] = "(", ")"
    return "".join(out)


def test_gpu_bit_equal_to_emulation(eng):
    rng = np.random.default_rng(8)
    hetero = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(64)]
    homo = [x + "&" + x for x in (_rand(rng, 17) for _ in range(64))]
    for seqs, n_emu in ((hetero, 16), (homo, 16)):
        E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
        # the emulation waits on thread rendezvous: a sample of each batch (the GPU batch itself is the full 64)
        for k, (e2, e12, st) in enumerate(cofold_subopt_many(seqs[:n_emu])):
            assert st == 0
            assert (int(E2[k]), (int(E12[k, 0]), int(E12[k, 1]))) == (e2, e12), seqs[k]


def test_gpu_vs_oracle_and_properties_long(eng, oracle):
    rng = np.random.default_rng(9)
    for la, lb in ((100, 100), (33, 90), (200, 200)):
        seqs = [_rand(rng, la) + "&" + _rand(rng, lb) for _ in range(6)]
        E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
        for k, s in enumerate(seqs):
            a, b = s.split("&")
            assert int(E12[k, 0]) == oracle.cofold_mfe(s)[1], s
            (a1, a2), (b1, b2) = oracle.two_best(a), oracle.two_best(b)
            assert int(E12[k, 0]) <= int(E12[k, 1]) <= min(a1 + b2, a2 + b1), s
            assert int(E2[k]) == _e2([int(x) for x in E12[k]])
    for L in (100, 200):
        # unconnected only: nothing joins {G, C} to A (no DuplexInit, every structure counted once)
        xs = [_rand(rng, L, "GC") for _ in range(4)]
        for seqs in ([x + "&" + "A" * L for x in xs], ["A" * L + "&" + x for x in xs]):
            E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
            for k, x in enumerate(xs):
                assert (int(E12[k, 0]), int(E12[k, 1])) == oracle.two_best(x), x
                assert int(E2[k]) == _e2(oracle.two_best(x))
        # homodimer rotation: an asymmetric ground state has its rotated twin as second structure of equal energy
        xs = []
        while len(xs) < 4:
            x = _rand(rng, L)
            db = oracle.cofold_mfe(x + "&" + x)[0].replace("&", "")
            if _rotate(db, L) != db:
                xs.append(x)
        E2, E12 = eng.cofold_subopt_energy([x + "&" + x for x in xs], want_both=True)
        for k, x in enumerate(xs):
            e = oracle.cofold_mfe(x + "&" + x)[1]
            assert (int(E12[k, 0]), int(E12[k, 1]), int(E2[k])) == (e, e, e), x
    E2, E12 = eng.cofold_subopt_energy(["AAAA&AAAA"], want_both=True)
    assert (int(E12[0, 0]), int(E12[0, 1]), int(E2[0])) == (0, INF_REF, 0)


def test_golden_two_strand_rows(eng, oracle, traj_golden):
    """E12[0] is the energy of the golden mfe_dimer structure, for all 708 two-strand rows"""
    rows = [r for r in traj_golden if r["run"] in ("RNA_RNA_complex_design_input", "Homodimer_design_input")]
    assert len(rows) == 708
    for b in range(0, len(rows), 128):
        chunk = rows[b:b + 128]
        by_shape = {}
        for r in chunk:
            sa, sb = r["sequence"].split("&")
            by_shape.setdefault((len(sa), len(sb)), []).append(r)      # one batch = one strand-length pair
        for (cut, _), rs in by_shape.items():
            E2, E12 = eng.cofold_subopt_energy([r["sequence"] for r in rs], want_both=True)
            for k, r in enumerate(rs):
                assert int(E12[k, 0]) == oracle.eval_structure(r["sequence"], r["mfe_ss"], cut), r["sequence"]
                assert int(E2[k]) == _e2([int(x) for x in E12[k]])


def test_scorer_two_strands_subopt(eng, traj_golden, example_inputs):
    """ReplicaScorer with -nd on and two strands: subopt_e = E2 / 100 for solved rows, the scoring function in the reference's
    order (scoring function, - (Esubopt - Epf), oligomer / monomer bonus), unsolved rows as with -nd off"""
    from desirna_amd.energy_scores import ReplicaScorer
    for run, state in (("RNA_RNA_complex_design_input", "heterodimer"), ("Homodimer_design_input", "homodimer")):
        tg = example_inputs[run]["sec_struct"][0]
        rows = [r for r in traj_golden if r["run"] == run]
        rows = [r for r in rows if float(r["one_minus_mcc"]) == 0][:24] + [r for r in rows if float(r["one_minus_mcc"]) > 0][:24]
        seqs = [r["sequence"] for r in rows]
        inp = SimpleNamespace(sec_struct=tg, alt_sec_struct=None, alt_sec_structs=None)
        mk = lambda nd: SimpleNamespace(oligo_state=state, subopt=nd, pks="off", scoring_f=[("Ed-Epf", 1.0)], motifs={}, param="1999")
        on = ReplicaScorer(inp, mk("on"), max_replicas=64, engine=eng).score(seqs)
        off = ReplicaScorer(inp, mk("off"), max_replicas=64, engine=eng).score(seqs)
        solved = [k for k, s in enumerate(on) if s.mcc == 0]
        assert 0 < len(solved) < len(seqs)
        E2 = eng.cofold_subopt_energy([seqs[k] for k in solved])
        for k, v in zip(solved, E2):
            s, o = on[k], off[k]
            assert s.subopt_e == int(v) / 100.0
            assert s.esubopt_minus_Epf == s.subopt_e - s.Epf
            want = o.edesired_minus_Epf * 1.0
            want = want - (s.subopt_e - s.Epf)
            want = want + s.oligomer_bonus
            assert s.scoring_function == want                         # bit for bit, the reference's order
        for k in set(range(len(seqs))) - set(solved):
            assert vars(on[k]) == vars(off[k])


def test_cli_two_strand_negative_design(tmp_path, example_inputs):
    for run, extra in (("RNA_RNA_complex_design_input", []), ("Homodimer_design_input", ["-d", "on"])):
        d = example_inputs[run]
        f = tmp_path / (run + ".txt")
        f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (d["name"][0].replace(" ", "_"), d["seq_restr"][0], d["sec_struct"][0]))
        out = tmp_path / ("out_" + run)
        p = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-nd", "on", "-R", "8", "-s", "3", "-e", "5",
                            "-o", str(out)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        assert any(n.endswith("_results.csv") for n in os.listdir(out)), os.listdir(out)


def test_errors(eng):
    from desirna_amd import engine as E
    with pytest.raises(E.EngineError) as ei:
        eng.cofold_subopt_energy(["GGGXAAAC&GUUUCCC"])
    assert ei.value.code == -4
    with pytest.raises(ValueError):
        eng.cofold_subopt_energy(["GGGAAAC&GUUUCCC", "GGGAAACC&GUUUCC"])
    rc = eng._L.drna_cofold_subopt_energy_batch(eng._h, 1, 8, 8, b"GGGAAACC", np.zeros(1, np.int32).ctypes.data, None)
    assert rc == -1
    rc = eng._L.drna_cofold_subopt_energy_batch(eng._h, 1, 8, 0, b"GGGAAACC", np.zeros(1, np.int32).ctypes.data, None)
    assert rc == -1
