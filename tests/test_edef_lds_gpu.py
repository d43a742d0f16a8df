"""Ensemble defect of short designs on the GPU through the fused LDS kernel (fold_edef_lds.hpp; option "edef_lds", default 1):
drna_ensemble_defect_batch, drna_cofold_ensemble_defect_batch and the Edef step of the native Monte-Carlo loops.

Two strands: the fused kernel runs the bodies of the general kernels, so option 1 against 0 is == on every number.  One strand
is the instance with an empty second strand in another order of summation than outside_kernel: checked against the oracle
within EDEF_TOL = 1e-10; the distance to the general path is printed, not asserted.  The counter "edef_lds_calls"
shows which path ran."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_cofold_edef_emulated import EDEF_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG36 = "((((((.((((((((....))))).)).).))))))"


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=64, max_L=100, device=0)
    yield e
    e.set_option("edef_lds", 1)
    e.close()


def _rand(rng, L, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), L))


def _both(eng, fn, seqs):
    """(result with the fused kernel, result with the general kernels, launches of the fused kernel in each)"""
    out, calls = [], []
    for lds in (1, 0):
        eng.set_option("edef_lds", lds)
        c0 = eng.get_option("edef_lds_calls")
        out.append(fn(seqs, want_bpp=True))
        calls.append(eng.get_option("edef_lds_calls") - c0)
    eng.set_option("edef_lds", 1)
    return out[0], out[1], calls


def _joining_target(la, lb, k):
    return "." * (la - k - 1) + "(" * k + "." + "." + ")" * k + "." * (lb - k - 1)


def test_bounds_cover_the_reference_examples(eng):
    assert eng.get_option("edef_lds_max") >= 36
    assert eng.get_option("cofold_edef_lds_max") >= 36
    assert eng.get_option("edef_lds") == 1


def test_two_strands_equal_the_general_kernels(eng, traj_golden, example_inputs):
    rng = np.random.default_rng(61)
    M = eng.get_option("cofold_edef_lds_max")
    hom = [r["sequence"] for r in traj_golden if r["run"] == "Homodimer_design_input"][:32]
    cases = [([_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(64)], _joining_target(18, 18, 6), True),
             (hom, example_inputs["Homodimer_design_input"]["sec_struct"][0].replace("&", ""), True),
             ([_rand(rng, M // 2, "GGCCAU") + "&" + _rand(rng, M - M // 2, "GGCCAU") for _ in range(16)], "." * M, True),
             ([_rand(rng, 1) + "&" + _rand(rng, M - 1) for _ in range(4)], "." * M, True),
             ([_rand(rng, M // 2 + 1, "GGCCAU") + "&" + _rand(rng, M - M // 2, "GGCCAU") for _ in range(8)], "." * (M + 1), False)]
    for seqs, tg, fits in cases:
        eng.set_targets([tg])
        (ed1, bpp1), (ed0, bpp0), calls = _both(eng, eng.cofold_ensemble_defect, seqs)
        assert calls == [1 if fits else 0, 0], (len(tg), calls)        # bound + 1: the general kernels, the counter stands still
        assert (ed1 == ed0).all() and (bpp1 == bpp0).all(), len(tg)
        assert ed1.min() >= 0.0 and ed1.max() <= 1.0 and bpp1.max() > 0.0


def test_one_strand_against_the_oracle(eng, oracle):
    rng = np.random.default_rng(62)
    M = eng.get_option("edef_lds_max")
    for L, tg, fits in ((5, ".....", True), (36, TG36, True), (M, "((((((" + "." * (M - 12) + "))))))", True),
                        (M + 1, "((((((" + "." * (M - 11) + "))))))", False)):
        seqs = [_rand(rng, L, "GGCCAU" if k % 2 else "ACGU") for k in range(8)]
        eng.set_targets([tg])
        (ed1, bpp1), (ed0, bpp0), calls = _both(eng, eng.ensemble_defect, seqs)
        assert calls == [1 if fits else 0, 0], (L, calls)
        dE = dP = 0.0
        for k, s in enumerate(seqs):
            oe, ob = oracle.ensemble_defect(s, tg, want_bpp=True)
            dE, dP = max(dE, abs(ed1[k] - oe)), max(dP, float(np.abs(bpp1[k] - ob).max()))
        print("L=%d: vs oracle max|dEdef| %.3e max|dP| %.3e; |LDS - general| Edef %.3e P %.3e"
              % (L, dE, dP, np.abs(ed1 - ed0).max(), np.abs(bpp1 - bpp0).max()))
        assert dE < EDEF_TOL and dP < EDEF_TOL, L
        assert (np.tril(bpp1) == 0.0).all() and (bpp1[:, 0] == 0.0).all()      # nothing outside 1 <= i < j <= L is written


def test_bits_do_not_depend_on_batch_or_engine(eng):
    from desirna_amd import engine
    rng = np.random.default_rng(63)
    pairs = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(64)]
    ones = [_rand(rng, 36) for _ in range(64)]
    eng.set_targets([TG36])
    c0 = eng.get_option("edef_lds_calls")
    p64, b64 = eng.cofold_ensemble_defect(pairs, want_bpp=True)
    o64 = eng.ensemble_defect(ones)
    p1, b1 = eng.cofold_ensemble_defect(pairs[37:38], want_bpp=True)
    assert p1[0] == p64[37] and (b1[0] == b64[37]).all()
    assert eng.ensemble_defect(ones[5:6])[0] == o64[5]
    mixed = eng.ensemble_defect(ones[40:] + ones[:3])                       # another batch composition
    assert (mixed == np.concatenate([o64[40:], o64[:3]])).all()
    assert (eng.cofold_ensemble_defect(pairs) == p64).all()                 # NULL bpp
    assert eng.get_option("edef_lds_calls") == c0 + 6
    small = engine.Engine(max_R=64, max_L=36, device=0)
    try:
        small.set_targets([TG36])
        assert (small.cofold_ensemble_defect(pairs) == p64).all() and (small.ensemble_defect(ones) == o64).all()
    finally:
        small.close()


def test_batch_larger_than_max_R():
    from desirna_amd import engine
    rng = np.random.default_rng(64)
    pairs = [_rand(rng, 17) + "&" + _rand(rng, 18) for _ in range(24)]
    ones = [_rand(rng, 36) for _ in range(24)]
    e = engine.Engine(max_R=8, max_L=36, device=0)
    try:
        for lds in (1, 0):
            e.set_option("edef_lds", lds)
            e.set_targets(["(((.(((((....))..(((....)))..))))))"])                 # the 17 + 18 example
            ed, bpp = e.cofold_ensemble_defect(pairs, want_bpp=True)
            parts = [e.cofold_ensemble_defect(pairs[k:k + 8], want_bpp=True) for k in (0, 8, 16)]
            assert (ed == np.concatenate([p[0] for p in parts])).all() and (bpp == np.concatenate([p[1] for p in parts])).all()
            e.set_targets([TG36])
            ed, bpp = e.ensemble_defect(ones, want_bpp=True)
            parts = [e.ensemble_defect(ones[k:k + 8], want_bpp=True) for k in (0, 8, 16)]
            assert (ed == np.concatenate([p[0] for p in parts])).all() and (bpp == np.concatenate([p[1] for p in parts])).all()
        assert e.get_option("edef_lds_calls") == 2 * (3 + 3)
        e.set_option("edef_lds", 1)
        with pytest.raises(engine.EngineError) as ei:
            e.ensemble_defect(ones[:19] + ["GGGANACC" + "A" * 28] + ones[20:])
        assert ei.value.code == -4 and "sequence 19" in str(ei.value)
    finally:
        e.close()


def test_gpu_against_emulation(eng):
    """same kernel source, same order of summation; 1e-12 is the bound tests/test_cofold_edef_gpu.py uses for what the two
    compilers contract into fused multiply-adds"""
    from tests.emu.emu_edef_lds import edef_lds_many
    rng = np.random.default_rng(65)
    pairs = [_rand(rng, 18) + "&" + _rand(rng, 18) for _ in range(4)]
    ones = [_rand(rng, 36) for _ in range(4)]
    tg2 = _joining_target(18, 18, 6)
    emu = edef_lds_many(pairs + ones, [tg2[:18] + "&" + tg2[18:]] * 4 + [TG36] * 4)
    assert all(x[3] == 0 for x in emu)
    eng.set_targets([tg2])
    ed2, bpp2 = eng.cofold_ensemble_defect(pairs, want_bpp=True)
    eng.set_targets([TG36])
    ed1, bpp1 = eng.ensemble_defect(ones, want_bpp=True)
    ed, bpp = np.concatenate([ed2, ed1]), np.concatenate([bpp2, bpp1])
    dE = max(abs(float(ed[k]) - emu[k][0]) for k in range(8))
    dP = max(float(np.abs(bpp[k] - emu[k][1]).max()) for k in range(8))
    print("GPU against emulation: max|dEdef| %.3e max|dP| %.3e" % (dE, dP))
    assert dE < 1e-12 and dP < 1e-12


def _inp(name, tg, restr):
    return SimpleNamespace(name=name, sec_struct=tg, seq_restr=restr, seed_seq=None, alt_sec_struct=None, alt_sec_structs=None)


@pytest.mark.parametrize("kind", ["one", "two"])
def test_native_loop_with_edef_term(kind, example_inputs, monkeypatch):
    """native loop == per-iteration loop with an Edef term, the Edef step on the fused kernel; two strands: the whole run is
    bit-equal between edef_lds 1 and 0"""
    from desirna_amd import design, engine
    from desirna_amd import energy_scores as es
    # more than one -sf term: the reference keeps the first only (parse_scoring_functions); all of them here
    monkeypatch.setattr(es, "parse_scoring_functions", lambda s, first_term_only=True, _p=es.parse_scoring_functions: _p(s, False))
    if kind == "one":
        inp, L = _inp("edef", TG36, "N" * 36), 36
    else:
        ex = example_inputs["RNA_RNA_complex_design_input"]
        inp, L = _inp("pair", ex["sec_struct"][0], ex["seq_restr"][0]), len(ex["sec_struct"][0]) - 1
    kw = dict(replicas=8, exchange=10, steps=3, seed=5, scoring_f="Ed-Epf:0.5,Edef:1.0")
    e = engine.Engine(max_R=8, max_L=L, device=0)
    try:
        a = design.run_design_fast(inp, native_loop=True, engine=e, **kw)
        calls = e.get_option("edef_lds_calls")
        assert calls > 0
        b = design.run_design_fast(inp, native_loop=False, engine=e, **kw)
        assert a["used_native_loop"] and not b["used_native_loop"]
        e.set_option("edef_lds", 0)
        c0 = e.get_option("edef_lds_calls")
        c = design.run_design_fast(inp, native_loop=True, engine=e, **kw)
        assert e.get_option("edef_lds_calls") == c0
    finally:
        e.close()
    key = lambda res, k: [r[k] for r in res["simulation_data"]]
    assert key(a, "sequence") == key(b, "sequence") and key(a, "scoring_function") == key(b, "scoring_function")
    for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
        assert a["stats"][k] == b["stats"][k], k
    if kind == "two":
        assert key(a, "sequence") == key(c, "sequence") and key(a, "scoring_function") == key(c, "scoring_function")
        assert key(a, "mfe_ss") == key(c, "mfe_ss")
        for k in ("acc_mc", "acc_mc_better", "rej_mc", "acc_re", "rej_re", "scored"):
            assert a["stats"][k] == c["stats"][k], k
    else:
        d = max(abs(x - y) for x, y in zip(key(a, "scoring_function"), key(c, "scoring_function")))
        print("one strand, edef_lds 1 against 0: max |d score| %.3e, same sequences: %s" % (d, key(a, "sequence") == key(c, "sequence")))


@pytest.mark.parametrize("run", ["Standard_design_input", "RNA_RNA_complex_design_input"])
def test_cli_edef(tmp_path, example_inputs, run):
    d = example_inputs[run]
    f = tmp_path / (run + ".txt")
    f.write_text(">name\n%s\n>seq_restr\n%s\n>sec_struct\n%s\n" % (d["name"][0].replace(" ", "_"), d["seq_restr"][0], d["sec_struct"][0]))
    p = subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-sf", "Edef:1.0", "-s", "2", "-R", "4"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    n = len(d["sec_struct"][0])
    assert any(len(w) == n and set(w) <= set("ACGU&") and w.count("&") == d["sec_struct"][0].count("&") for w in p.stdout.split()), p.stdout[-2000:]


def test_errors(eng):
    from desirna_amd import engine as E
    eng.set_targets(["." * 15])
    for call in (lambda: eng.cofold_ensemble_defect(["GGGAAAAC&GUUUCCC", "GGGXAAAC&GUUUCCC"]),
                 lambda: eng.ensemble_defect(["GGGAAAACGUUUCCC", "GGGXAAACGUUUCCC"])):
        c0 = eng.get_option("edef_lds_calls")
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == -4 and eng.get_option("edef_lds_calls") == c0 + 1
    ed = np.zeros(1)
    call = lambda L, cut, seq: eng._L.drna_cofold_ensemble_defect_batch(eng._h, 1, L, cut, seq, ed.ctypes.data, None)
    assert call(15, 8, b"GGGAAACCGUUUCCC") == 0 and 0.0 < ed[0] < 1.0                          # NULL bpp accepted
    assert eng._L.drna_ensemble_defect_batch(eng._h, 1, 15, b"GGGAAACCGUUUCCC", ed.ctypes.data, None) == 0
    assert call(15, 15, b"GGGAAACCGUUUCCC") == -1 and call(15, 0, b"GGGAAACCGUUUCCC") == -1      # the empty second strand stays internal
    assert eng._L.drna_ensemble_defect_batch(eng._h, 0, 15, b"", ed.ctypes.data, None) == -1
    with pytest.raises(E.EngineError):
        eng.set_option("edef_lds_max", 80)                                                       # read-only
