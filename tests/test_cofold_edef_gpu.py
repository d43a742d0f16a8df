"""Two-strand pair probabilities and ensemble defect on the GPU (drna_cofold_ensemble_defect_batch, cofold_outside_kernel):
-sf Edef and -sf Ed-MFE for heterodimer / homodimer designs.

The reference holds no value here.  This file checks the GPU against the CPU emulation of the same kernel source (which
tests/test_cofold_edef_emulated.py checks against exhaustive enumeration), against the identities that follow from the
definition, and through the scorer and the command line.  The independent values at lengths the enumeration cannot
reach (1+1 to 150+250) are in tests/test_pair_prob_reference_gpu.py: pair probabilities from forbidden-pair free energies of the
oracle's inside fill (tests/pair_prob_ref.py)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests.emu.emu import cofold_edef_many
from tests.test_cofold_edef_emulated import EDEF_TOL, PAIRS, defect_from_matrix

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


def _random_target(rng, la, lb):
    """a nested target over both strands: a few joining pairs around the nick, dots elsewhere"""
    k = int(rng.integers(1, min(la, lb) // 2 + 1))
    a = ["."] * la
    b = ["."] * lb
    for x in range(k):
        a[la - 1 - x - 1] = "("
        b[x + 1] = ")"
    return "".join(a) + "&" + "".join(b)


def test_gpu_against_emulation(eng):
    """same kernel source, same order of summation: the bits are expected to agree up to what the two compilers contract into
    fused multiply-adds, so the bound is 1e-12 (measured figures are printed before the assertion)"""
    rng = np.random.default_rng(21)
    for la, lb in ((18, 18), (25, 11), (50, 50)):
        seqs = [_rand(rng, la) + "&" + _rand(rng, lb) for _ in range(8)]
        tg = _random_target(rng, la, lb)
        eng.set_targets([tg.replace("&", "")])
        ed, bpp = eng.cofold_ensemble_defect(seqs, want_bpp=True)
        emu = cofold_edef_many(seqs, [tg] * len(seqs))
        dP = max(float(np.abs(bpp[k] - emu[k][1]).max()) for k in range(len(seqs)))
        dE = max(abs(float(ed[k]) - emu[k][0]) for k in range(len(seqs)))
        print("%d+%d: max|dP| %.3e max|dEdef| %.3e bit-equal %s" % (la, lb, dP, dE, dP == 0.0 and dE == 0.0))
        assert all(e[3] == 0 for e in emu)
        assert dP < 1e-12 and dE < 1e-12, (la, lb)


def test_bits_do_not_depend_on_batch_or_engine(eng):
    from desirna_amd import engine
    rng = np.random.default_rng(22)
    seqs = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(64)]
    tg = "." * 36
    eng.set_targets([tg])
    ed64, bpp64 = eng.cofold_ensemble_defect(seqs, want_bpp=True)
    ed1, bpp1 = eng.cofold_ensemble_defect(seqs[37:38], want_bpp=True)
    assert ed1[0] == ed64[37] and (bpp1[0] == bpp64[37]).all()
    small = engine.Engine(max_R=64, max_L=36, device=0)
    try:
        small.set_targets([tg])
        ed_s, bpp_s = small.cofold_ensemble_defect(seqs, want_bpp=True)
    finally:
        small.close()
    assert (ed_s == ed64).all() and (bpp_s == bpp64).all()
    assert (eng.cofold_ensemble_defect(seqs) == ed64).all()              # NULL bpp, and a second call on the used workspace


def test_strands_that_cannot_pair(eng, oracle):
    rng = np.random.default_rng(23)
    for L in (30, 100):
        xs = [_rand(rng, L, "GC") for _ in range(4)]
        for mirrored in (False, True):
            lb = L // 2
            seqs = [("A" * lb + "&" + x) if mirrored else (x + "&" + "A" * lb) for x in xs]
            eng.set_targets(["." * (L + lb)])
            ed, bpp = eng.cofold_ensemble_defect(seqs, want_bpp=True)
            off = lb if mirrored else 0
            for k, x in enumerate(xs):
                ed1, P1 = oracle.ensemble_defect(x, "." * L, want_bpp=True)
                want = np.zeros_like(bpp[k])
                want[off + 1:off + L + 1, off + 1:off + L + 1] = P1[1:, 1:]
                assert np.abs(bpp[k] - want).max() < EDEF_TOL, (x, mirrored)


def _check_matrix(flat, cut, P):
    n = len(flat)
    assert P.min() >= 0.0 and P.max() <= 1.0
    S = P + P.T
    assert S.sum(1).max() <= 1.0 + 1e-12
    ok = np.zeros((n + 1, n + 1), dtype=bool)
    for i in range(1, n + 1):
        for j in range(i + 1, n + 1):
            ok[i, j] = flat[i - 1] + flat[j - 1] in PAIRS and (i <= cut < j or j - i >= 4)
    assert P[~ok].max() == 0.0


def test_identities_long(eng):
    rng = np.random.default_rng(24)
    for la, lb in ((40, 60), (100, 100)):
        seqs = [_rand(rng, la) + "&" + _rand(rng, lb) for _ in range(4)]
        eng.set_targets(["." * (la + lb)])
        ed, bpp = eng.cofold_ensemble_defect(seqs, want_bpp=True)
        for k, s in enumerate(seqs):
            _check_matrix(s.replace("&", ""), la, bpp[k])
            assert abs(ed[k] - (bpp[k] + bpp[k].T)[1:, 1:].sum() / (la + lb)) < EDEF_TOL
    for L in (30, 100):                                     # homodimer: rotation by cut maps the ensemble onto itself
        xs = [_rand(rng, L) for _ in range(4)]
        eng.set_targets(["." * (2 * L)])
        ed, bpp = eng.cofold_ensemble_defect([x + "&" + x for x in xs], want_bpp=True)
        for k in range(len(xs)):
            P = bpp[k]
            assert np.abs(P[1:L + 1, 1:L + 1] - P[L + 1:, L + 1:]).max() < EDEF_TOL
            J = P[1:L + 1, L + 1:]                          # J[i-1, j-cut-1] = P(i, j) = P(j-cut, i+cut) = J[j-cut-1, i-1]
            assert np.abs(J - J.T).max() < EDEF_TOL and J.max() > 0


def test_golden_two_strand_rows(eng, traj_golden, example_inputs):
    """the reference's own 18+18 rows: ranges, structural zeros, and the defect recomputed from the returned matrix.  The values
    themselves at 18+18 are held to an independent reference in tests/test_pair_prob_reference_gpu.py"""
    for run in ("RNA_RNA_complex_design_input", "Homodimer_design_input"):
        tg = example_inputs[run]["sec_struct"][0]
        rows = [r for r in traj_golden if r["run"] == run][:64]
        assert len(rows) == 64
        seqs = [r["sequence"] for r in rows]
        cut = len(seqs[0].split("&")[0])
        eng.set_targets([tg.replace("&", "")])
        ed, bpp = eng.cofold_ensemble_defect(seqs, want_bpp=True)
        for k, s in enumerate(seqs):
            _check_matrix(s.replace("&", ""), cut, bpp[k])
            assert 0.0 <= ed[k] <= 1.0
            assert abs(ed[k] - defect_from_matrix(bpp[k], tg)) < 1e-12, s


def test_scorer_two_strands_edef_and_ed_mfe(eng, traj_golden, example_inputs):
    from desirna_amd.energy_scores import ReplicaScorer
    for run, state in (("RNA_RNA_complex_design_input", "heterodimer"), ("Homodimer_design_input", "homodimer")):
        tg = example_inputs[run]["sec_struct"][0]
        seqs = [r["sequence"] for r in traj_golden if r["run"] == run][:32]
        inp = SimpleNamespace(sec_struct=tg, alt_sec_struct=None, alt_sec_structs=None)
        mk = lambda sf: SimpleNamespace(oligo_state=state, subopt="off", pks="off", scoring_f=[(sf, 1.0)], motifs={}, param="1999")
        res = ReplicaScorer(inp, mk("Edef"), max_replicas=64, engine=eng).score(seqs)
        want = eng.cofold_ensemble_defect(seqs)
        for k, s in enumerate(res):
            assert s.ensemble_defect == float(want[k])
            assert s.scoring_function == s.ensemble_defect * 1.0 + s.oligomer_bonus
        res = ReplicaScorer(inp, mk("Ed-MFE"), max_replicas=64, engine=eng).score(seqs)
        co = eng.cofold_batch(seqs)
        for k, s in enumerate(res):
            assert s.MFE == int(co["Emfe"][k]) / 100.0
            assert s.edesired_minus_MFE == s.edesired - int(co["Emfe"][k]) / 100.0
            assert s.scoring_function == s.edesired_minus_MFE * 1.0 + s.oligomer_bonus


def test_cli_two_strand_edef(tmp_path, example_inputs):
    for run, extra in (("RNA_RNA_complex_design_input", []), ("Homodimer_design_input", ["-d", "on"])):
        d = example_inputs[run]
        f = tmp_path / (run + ".txt")
        f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (d["name"][0].replace(" ", "_"), d["seq_restr"][0], d["sec_struct"][0]))
        p = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-sf", "Edef:1.0", "-s", "2", "-R", "4"] + extra,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        la, lb = (len(x) for x in d["sec_struct"][0].split("&"))
        lines = p.stdout.split()
        assert any(len(w) == la + lb + 1 and w[la] == "&" and set(w) <= set("ACGU&") for w in lines), p.stdout[-2000:]


def test_errors(eng):
    from desirna_amd import engine as E
    eng.set_targets(["." * 15])
    with pytest.raises(E.EngineError) as ei:
        eng.cofold_ensemble_defect(["GGGXAAAC&GUUUCCC"])
    assert ei.value.code == -4
    with pytest.raises(ValueError):
        eng.cofold_ensemble_defect(["GGGAAAC&GUUUCCC", "GGGAAACC&GUUUCC"])
    ed = np.zeros(1)
    call = lambda L, cut, seq: eng._L.drna_cofold_ensemble_defect_batch(eng._h, 1, L, cut, seq, ed.ctypes.data, None)
    assert call(15, 8, b"GGGAAACCGUUUCCC") == 0                     # NULL bpp accepted
    assert call(15, 15, b"GGGAAACCGUUUCCC") == -1 and call(15, 0, b"GGGAAACCGUUUCCC") == -1
    assert call(14, 7, b"GGGAAACGUUUCCC") == -1                      # L differs from the targets' L
    fresh = E.Engine(max_R=1, max_L=15, device=0)
    try:
        assert fresh._L.drna_cofold_ensemble_defect_batch(fresh._h, 1, 15, 8, b"GGGAAACCGUUUCCC", ed.ctypes.data, None) == -1   # no targets
        fresh.set_targets(["((((.......))))"])
        assert fresh.cofold_ensemble_defect(["GGGAAACC&GUUUCCC"]).shape == (1,)      # one slot at max_L: the tables still fit
    finally:
        fresh.close()
