"""Stochastic traceback on the GPU (Engine.sample_structures: pf_kernel<1024> + sample_kernel<256>): exact structure probabilities
by enumeration, pair frequencies against the forbidden-pair reference AND the engine's own outside recursion, energies against
the oracle, determinism across calls, batch compositions and chunks, the same samples as the CPU emulation for the same seeds,
the error codes, and one command-line run with --ensemble.  The comparison rule and the references: tests/sampling_ref.py."""
import csv

import numpy as np
import pytest

from tests import pair_prob_ref as ppr
from tests import sampling_ref as sr
from tests.test_sampling_emulated import MULTILOOP, SHORT

pytestmark = pytest.mark.gpu

MAX_R = 8
ERR_ARG, ERR_SEQUENCE = -1, -4


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=MAX_R, max_L=201, device=0)
    yield e
    e.close()


def test_exact_distribution(eng, oracle):
    seqs, S = [SHORT[0], SHORT[2]], 20000
    c0 = eng.get_option("sample_calls")
    ss, E, Epf = eng.sample_structures(seqs, S, seed=100)
    assert eng.get_option("sample_calls") == c0 + 1
    for r, seq in enumerate(seqs):
        dist = sr.exact_distribution(oracle, seq)
        bad = sr.check_distribution(ss[r], dist)
        assert not bad, bad
        assert abs(Epf[r] - oracle.pf(seq)) < 1e-6
        for s in set(ss[r]):
            assert E[r, ss[r].index(s)] == oracle.eval_structure(seq, s)


def test_multiloop_distribution(eng, oracle):
    ss, _, _ = eng.sample_structures([MULTILOOP], 20000, seed=105)
    bad = sr.check_distribution(ss[0], sr.exact_distribution(oracle, MULTILOOP))
    assert not bad, bad


@pytest.mark.parametrize("L", [70, 130, 201])
def test_pair_frequencies_and_energies(eng, oracle, L):
    S = 4096
    seq = ppr.rand_seq(np.random.default_rng(L), L)
    ss, E, Epf = eng.sample_structures([seq], S, seed=L)
    ss = ss[0]
    assert all(sr.well_formed(seq, s) for s in set(ss))
    for s in set(ss):
        assert E[0, ss.index(s)] == oracle.eval_structure(seq, s)
    pairs = ppr.allowed_pairs(seq)
    P = ppr.reference_matrix(oracle, seq, pairs)
    bad = sr.check_pair_frequencies(ss, P, pairs)
    assert not bad, bad
    eng.set_targets(["." * L])
    _, bpp = eng.ensemble_defect([seq], want_bpp=True)
    bad = sr.check_pair_frequencies(ss, bpp[0], pairs)
    assert not bad, bad
    assert abs(Epf[0] - oracle.pf(seq)) < 1e-6


def test_determinism_batches_and_chunks(eng):
    rng = np.random.default_rng(7)
    seqs = [ppr.rand_seq(rng, 40) for _ in range(3 * MAX_R)]
    seeds = np.arange(1000, 1000 + len(seqs), dtype=np.uint64)
    S = 48
    a = eng.sample_structures_arrays(np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1), S, seeds)
    b = eng.sample_structures_arrays(np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1), S, seeds)
    assert a[0].all() and (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()      # two calls; R = 3 max_R: chunks
    # another composition: a few of them, in another order, more samples
    pick = [17, 3, 9]
    ss, E, _ = eng.sample_structures([seqs[k] for k in pick], 2 * S, seeds[pick])
    for row, k in enumerate(pick):
        want = [bytes(x).decode() for x in a[0][k]]
        assert ss[row][:S] == want and (E[row, :S] == a[1][k]).all()
    # an integer seed gives sequence r the seed seed + r
    ss2, _, _ = eng.sample_structures(seqs[:2], S, seed=1000)
    assert ss2[0] == [bytes(x).decode() for x in a[0][0]] and ss2[1] == [bytes(x).decode() for x in a[0][1]]
    ss3, _, _ = eng.sample_structures(seqs[:1], S, seed=1001)
    assert ss3[0] != ss2[0]


def test_gpu_against_the_emulation(eng, eterna_solutions):
    """same seeds, same strings.  The two sets of tables agree to about 1e-12 only, so a draw may land between them: at most 0.1 %
    of the samples may differ (a condition; the expected count is 0)"""
    from tests.emu import emu_sampling as es
    from tests.test_sampling_emulated import long_cases
    cases = [([SHORT[0]], 2048, 31), ([MULTILOOP], 1024, 32), ([long_cases(eterna_solutions)[0]], 512, 33)]
    emu = es.sample_many(cases, G=8)
    differ = total = 0
    for (seqs, S, seed), r in zip(cases, emu):
        ss, E, _ = eng.sample_structures_arrays(np.frombuffer(seqs[0].encode(), dtype=np.uint8).reshape(1, -1), S, seed)
        same = (ss == r["ss"]).all(axis=2)
        differ += int((~same).sum())
        total += same.size
        assert (E[same] == r["E"][same]).all()
    print("GPU against emulation: %d of %d samples differ" % (differ, total))
    assert differ <= total // 1000


def test_error_codes(eng):
    import ctypes as C
    from desirna_amd.engine import EngineError
    good, bad = SHORT[0], "GGACGAAXGCAAAACC"
    with pytest.raises(EngineError) as ex:
        eng.sample_structures([good, bad, good], 8)
    assert ex.value.code == ERR_SEQUENCE and "sequence 1" in str(ex.value)
    with pytest.raises(EngineError) as ex:
        eng.sample_structures([good], 0)
    assert ex.value.code == ERR_ARG
    # R x S x L beyond the documented limit (1 << 30): refused before anything is written
    seeds = np.zeros(1, dtype=np.uint64)
    buf = np.zeros(16, dtype=np.uint8)
    rc = eng._L.drna_sample_structures_batch(eng._h, 1, 16, good.encode(), (1 << 26) + 1, seeds.ctypes.data, buf.ctypes.data, None, None)
    assert rc == ERR_ARG and not buf.any()
    rc = eng._L.drna_sample_structures_batch(eng._h, 1, 16, good.encode(), 4, None, buf.ctypes.data, None, None)
    assert rc == ERR_ARG
    ss, _, _ = eng.sample_structures([good], 4)                 # the engine is fine afterwards
    assert all(sr.well_formed(good, s) for s in ss[0])


def test_cli_run_with_ensemble(tmp_path):
    from desirna_amd import design, outputs
    target = "((((......))))"
    f = tmp_path / "hp.txt"
    f.write_text(">name\nhp\n>seq_restr\n%s\n>sec_struct\n%s\n" % ("N" * 14, target))
    out = tmp_path / "out"
    design.main(["-f", str(f), "-R", "4", "-s", "2", "--ensemble", "256", "-o", str(out)])
    (res_file,) = [p for p in out.iterdir() if p.name.endswith("_results.csv")]
    (ens_file,) = [p for p in out.iterdir() if p.name.endswith("_ensemble.csv")]
    reported = [r["sequence"] for r in csv.DictReader(open(res_file))]
    rows = list(csv.DictReader(open(ens_file)))
    assert tuple(rows[0].keys()) == outputs.ENSEMBLE_COLUMNS
    assert [r["sequence"] for r in rows if r["kind"] == "other"] == reported
    for seq in reported:
        mine = [r for r in rows if r["sequence"] == seq]
        top = [r for r in mine if r["kind"] == "top"]
        (tg,) = [r for r in mine if r["kind"] == "target"]
        (other,) = [r for r in mine if r["kind"] == "other"]
        assert 1 <= len(top) <= 5 and tg["structure"] == target
        in_top = target in [r["structure"] for r in top]
        assert sum(int(r["count"]) for r in top) + int(other["count"]) + (0 if in_top else int(tg["count"])) == 256
        assert all(sr.well_formed(seq, r["structure"]) for r in top)
