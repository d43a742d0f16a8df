"""K lowest-energy co-fold structures on the GPU (drna_cofold_subopt_structs_batch, cofold_kbest_kernel): the final ranking of a
two-strand design with alternative structures.

The reference pins no ranked structure for two strands; the GPU is checked byte for byte against the CPU emulation of the same
kernel source (which tests/test_cofold_kbest_emulated.py checks against exhaustive enumeration), against the co-fold MFE and the
second-best co-fold energy of the engine, and by re-evaluating every returned string with the oracle at lengths the emulation
cannot reach."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cofold_kbest_cases as cases
from tests.emu.emu_cofold_kbest import INF_REF

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


def _by_shape(seqs):
    """indices of the pairs with the same strand lengths (one call each)"""
    groups = {}
    for k, s in enumerate(seqs):
        groups.setdefault((s.index("&"), len(s)), []).append(k)
    return groups.values()


def _structs(eng, seqs, K):
    """eng.cofold_subopt_structs over pairs of any strand lengths -> [(E list, strings), ...] in the order of seqs"""
    out = [None] * len(seqs)
    for idx in _by_shape(seqs):
        E, ss = eng.cofold_subopt_structs([seqs[k] for k in idx], K)
        for row, k in enumerate(idx):
            out[k] = ([int(e) for e in E[row]], ss[row])
    return out


def _check_strings(oracle, s, E, ss):
    cut, flat = s.index("&"), s.replace("&", "")
    assert E == sorted(E), (s, E)
    fin = [x for e, x in zip(E, ss) if e < INF_REF]
    assert len(set(fin)) == len(fin), (s, fin)
    for e, x in zip(E, ss):
        assert len(x) == len(s) and x[cut] == "&"
        db = x.replace("&", "")
        if e >= INF_REF:
            assert db == "." * len(flat)
            continue
        depth = 0
        for ch in db:
            depth += (ch == "(") - (ch == ")")
            assert depth >= 0 and ch in "()."
        assert depth == 0, (s, x)
        assert oracle.eval_structure(flat, db, cut) == e, (s, x, e)


def test_gpu_byte_equal_to_emulation(eng):
    """the 60 enumeration pairs, rows of the golden shapes 17+18 and 17+17, 1+1, 1+35, 35+1 and one X&X against the emulated
    kernel's answers.  Those come from the record tests/golden/cofold_kbest_emulated.json (emulating a pair takes seconds), which
    tests/test_cofold_kbest_emulated.py holds to what the kernel source in the tree gives."""
    seqs, emu = cases.load()
    assert seqs == cases.pairs()
    assert {(17, 18), (17, 17), (1, 1), (1, 35), (35, 1), (13, 13)} <= {(s.index("&"), len(s) - 1 - s.index("&")) for s in seqs}
    # the emulation runs the two kernel instances (lists of 4 and of 8); K = 3 is the call's cut of the 4-list
    for K in (3, 4, 8):
        got = _structs(eng, seqs, K)
        for s, (E, ss), (Ee, sse) in zip(seqs, got, emu[4 if K <= 4 else 8]):
            assert (E, ss) == (Ee[:K], sse[:K]), (s, K)


@pytest.mark.parametrize("la,R,K", [(18, 8, 8), (50, 8, 8), (100, 2, 4)])
def test_energies_and_strings_long(eng, oracle, la, R, K):
    rng = np.random.default_rng(40 + la)
    seqs = [_rand(rng, la) + "&" + _rand(rng, la) for _ in range(R - 1)]
    x = _rand(rng, la, "GGCCAU")
    seqs.append(x + "&" + x)
    E, ss = eng.cofold_subopt_structs(seqs, K)
    from desirna_amd import engine
    mfe = eng.cofold_batch(seqs, flags=engine.NEED_MFE)["Emfe"]
    E2, E12 = eng.cofold_subopt_energy(seqs, want_both=True)
    for k, s in enumerate(seqs):
        row = [int(e) for e in E[k]]
        assert row[0] == int(mfe[k]), s
        assert row[:2] == [int(E12[k, 0]), int(E12[k, 1])], s
        assert row == oracle.kbest_energies(s, K), s                   # every rank: the oracle's serial K-list fill
        assert row[K - 1] < INF_REF, s                                 # (random pairs of this size have far more than K structures)
        _check_strings(oracle, s, row, ss[k])


def test_batch_and_engine_size(eng):
    """R = 1 against R = 20 (more than one chunk of the K-best workspace), an engine of max_L 36 against one of 400"""
    from desirna_amd import engine
    rng = np.random.default_rng(52)
    seqs = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(20)]
    small = engine.Engine(max_R=4, max_L=36, device=0)
    try:
        for K in (4, 8):
            E, ss = eng.cofold_subopt_structs(seqs, K)
            for k in (0, 15, 16, 19):
                E1, ss1 = eng.cofold_subopt_structs(seqs[k:k + 1], K)
                assert E1.tobytes() == E[k:k + 1].tobytes() and ss1[0] == ss[k], (K, k)
            Es, sss = small.cofold_subopt_structs(seqs, K)              # chunks of 4
            assert Es.tobytes() == E.tobytes() and sss == ss, K
    finally:
        small.close()


def test_both_orders_of_first_use():
    """the one-strand and the two-strand call share one workspace slot: whichever comes first, neither disturbs the other"""
    from desirna_amd import engine
    rng = np.random.default_rng(53)
    one = [_rand(rng, 36) for _ in range(5)]
    two = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(5)]
    res = []
    for first in ("one", "two"):
        e = engine.Engine(max_R=8, max_L=36, device=0)
        try:
            if first == "one":
                a = e.subopt_structs(one, 8)
                b = e.cofold_subopt_structs(two, 8)
            else:
                b = e.cofold_subopt_structs(two, 8)
                a = e.subopt_structs(one, 8)
            a2 = e.subopt_structs(one, 8)
            b2 = e.cofold_subopt_structs(two, 8)
            a4 = e.subopt_structs(one, 3)
        finally:
            e.close()
        assert a[0].tobytes() == a2[0].tobytes() and a[1] == a2[1]
        assert b[0].tobytes() == b2[0].tobytes() and b[1] == b2[1]
        assert a4[0].tobytes() == a[0][:, :3].copy().tobytes() and a4[1] == [row[:3] for row in a[1]]
        res.append((a[0].tobytes(), a[1], b[0].tobytes(), b[1]))
    assert res[0] == res[1]


@pytest.mark.parametrize("extra", [[], ["-d", "on"]])
def test_cli_two_strand_alt_design_writes_its_files(tmp_path, extra):
    """a two-strand design with an alternative structure, end to end in a fresh process: the final ranking takes the ranked co-fold
    structures and the result files carry mcc_1 / alt_struct_1"""
    f = tmp_path / "pair_alt.txt"
    target, alt = "(((((.((....&....)).)))))", "(((((..((...&....)).)))))"
    f.write_text(">name\npair_alt\n>seq_restr\n%s\n>sec_struct\n%s\n>alt_sec_struct\n%s\n" % ("N" * 12 + "&" + "N" * 12, target, alt))
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-R", "4", "-e", "5", "-s", "2", "-o", str(out)] + extra,
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    names = os.listdir(out)
    for suffix in ("_results.csv", "_traj.csv"):
        hit = [n for n in names if n.endswith(suffix)]
        assert len(hit) == 1, (suffix, names)
        rows = list(csv.DictReader(open(out / hit[0])))
        assert rows and "mcc_1" in rows[0] and "alt_struct_1" in rows[0], (suffix, list(rows[0]) if rows else None)
        for r in rows:
            assert len(r["alt_struct_1"]) == len(r["sequence"]) == 25, r
            assert r["alt_struct_1"][12] in "&." and 0.0 <= float(r["mcc_1"]) <= 2.0, r


def test_argument_errors(eng):
    from desirna_amd import engine as EG
    E = np.zeros(8, np.int32)
    ss = np.zeros(8 * 8, np.uint8)
    call = lambda L, cut, seq, K: eng._L.drna_cofold_subopt_structs_batch(eng._h, 1, L, cut, seq, K, E.ctypes.data, ss.ctypes.data)
    err = lambda: eng._L.drna_last_error(eng._h).decode()
    for cut in (0, 8):
        assert call(8, cut, b"GGGAAACC", 4) == -1
        assert "drna_cofold_subopt_structs_batch" in err() and "cut" in err()
    for K in (0, 9):
        assert call(8, 4, b"GGGAAACC", K) == -1
        assert "K" in err()
    assert call(8, 4, b"GGGAXACC", 4) == -4
    assert "sequence 0" in err()
    # the caller's index, also beyond the first chunk of the workspace
    seqs = ["GGGAAC&GUUCCC"] * 17 + ["GGGXAC&GUUCCC"]
    with pytest.raises(EG.EngineError) as ei:
        eng.cofold_subopt_structs(seqs, 2)
    assert ei.value.code == -4 and "sequence 17" in str(ei.value)
    with pytest.raises(ValueError):
        eng.cofold_subopt_structs(["GGGAAAC&GUUUCCC", "GGGAAACC&GUUUCC"], 2)
    assert call(8, 4, b"GGGAAACC", 4) == 0                             # the engine goes on after an error
