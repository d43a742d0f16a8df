"""Two-strand stochastic traceback on the GPU (Engine.cofold_sample_structures: cofold_pf_kernel<1024> + cofold_columns_kernel<256>
+ cofold_sample_kernel<256>): exact structure probabilities by enumeration of every co-fold structure, connected fractions,
energies against the oracle, the same samples as the CPU emulation for the same seeds, 100+100 nt and a fully stacked 60+60
duplex, a strand of one nucleotide, the same bytes whatever the batch, the chunks, the engine's limits and "cofold_lds", the error
codes and the counter.  The comparison rule and the references: tests/sampling_ref.py, tests/cofold_sampling_ref.py."""
import math

import numpy as np
import pytest

from tests import cofold_sampling_ref as cr
from tests import pair_prob_ref as ppr
from tests import sampling_ref as sr
from tests.test_cofold_sampling_emulated import LONG, long_case

pytestmark = pytest.mark.gpu

MAX_R = 64
ERR_ARG, ERR_SEQUENCE, ERR_PF_RANGE = -1, -4, -6
EXACT = ["UAGAUUAC&AGAA", "GCUUAAAC&UUAGAACC", cr.MULTILOOP, "GGUGUUA&GGUGUUA", "A&U"]


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=MAX_R, max_L=400, device=0)
    yield e
    e.close()


def check_energies(oracle, pair, ss, E):
    flat, cut = ppr.split(pair)
    for s in set(ss):
        assert E[ss.index(s)] == oracle.eval_structure(flat, s.replace("&", ""), cut), (pair, s)


def check_connected(ss, F4):
    f, p = sum(cr.is_connected(s) for s in ss) / len(ss), math.exp(-(F4[2] - F4[3]) / sr.KT)
    assert sr.meets(f, p, len(ss)), (f, p)


@pytest.mark.parametrize("pair", EXACT)
def test_exact_distribution(eng, oracle, pair):
    S = 20000
    c0 = eng.get_option("cofold_sample_calls")
    ss, E, F4 = eng.cofold_sample_structures([pair], S, seed=100)
    assert eng.get_option("cofold_sample_calls") == c0 + 1
    dist, F = cr.exact_distribution(oracle, pair)
    assert cr.enters(oracle, pair, F)
    assert len(ss[0]) == S
    bad = sr.check_distribution(ss[0], dist, p_min=0.0 if len(dist) == 2 else 1e-3)
    assert not bad, bad
    assert np.abs(F4[0] - np.array(oracle.cofold_pf(pair))).max() < 1e-6
    f_conn = sum(cr.is_connected(s) for s in ss[0]) / S
    assert sr.meets(f_conn, cr.connected_fraction(oracle, pair), S)
    check_energies(oracle, pair, ss[0], E[0])
    if pair.split("&")[0] == pair.split("&")[1]:
        assert all(abs(dist[cr.rotated(s)] - p) < 1e-12 for s, p in dist.items())


def test_gpu_against_the_emulation(eng):
    """same seeds, same strings.  The two compilers' tables agree to about 1e-12 only, so a draw may land between them: at most
    0.1 % of the samples may differ (a condition; the expected count is 0)"""
    from tests.emu import emu_cofold_sampling as ec
    cases = [([long_case(shape, cs)], 256, 40 + k) for k, (shape, cs, _) in enumerate(LONG)]
    emu = ec.sample_many(cases, G=8)
    differ = total = 0
    for (pairs, S, seed), r in zip(cases, emu):
        ss, E, _ = eng.cofold_sample_structures(pairs, S, seed)
        want = ec.strings(r["ss"], r["cut"])[0]
        same = np.array([a == b for a, b in zip(ss[0], want)])
        differ += int((~same).sum())
        total += same.size
        assert (E[0][same] == r["E"][0][same]).all()
    print("GPU against emulation: %d of %d samples differ" % (differ, total))
    assert differ <= total // 1000


@pytest.mark.parametrize("pair", [long_case((100, 100), 300), "G" * 60 + "&" + "C" * 60], ids=["planted100", "gc60"])
def test_long_pairs(eng, oracle, pair):
    S = 512
    ss, E, F4 = eng.cofold_sample_structures([pair], S, seed=7)
    ss = ss[0]
    assert len(ss) == S and all(cr.well_formed(pair, s) for s in set(ss))        # balanced, canonical pairs
    check_energies(oracle, pair, ss, E[0])
    assert np.abs(F4[0] - np.array(oracle.cofold_pf(pair))).max() < 1e-6
    check_connected(ss, F4[0])
    if pair.startswith("G" * 60):
        assert "(" * 60 + "&" + ")" * 60 in ss         # the deepest nesting: 60 PAIR steps on top of each other


@pytest.mark.parametrize("shape", [(1, 30), (30, 1)])
def test_a_strand_of_one_nucleotide(eng, oracle, shape):
    S = 2048
    pair = ppr.two_strand_case(np.random.default_rng(sum(shape) + shape[0]), shape[0], shape[1], "ACGU", True)
    ss, E, F4 = eng.cofold_sample_structures([pair], S, seed=3)
    assert all(cr.well_formed(pair, s) for s in set(ss[0]))
    check_energies(oracle, pair, ss[0], E[0])
    assert np.abs(F4[0] - np.array(oracle.cofold_pf(pair))).max() < 1e-6
    check_connected(ss[0], F4[0])
    pairs = ppr.allowed_pairs(pair)
    bad = sr.check_pair_frequencies([s.replace("&", "") for s in ss[0]], ppr.reference_matrix(oracle, pair, pairs), pairs)
    assert not bad, bad


def test_same_bytes_whatever_the_call(eng, monkeypatch):
    """R = 1 and R = 64, an engine whose workspace forces several chunks, engines of max_L 64 and 400, "cofold_lds" 0 and 1"""
    from desirna_amd import engine as E
    rng = np.random.default_rng(18)
    pairs = [ppr.two_strand_case(rng, 18, 18, "ACGU", k % 2 == 1) for k in range(MAX_R)]
    seeds = np.arange(500, 500 + MAX_R, dtype=np.uint64)
    S = 32
    eng.set_option("cofold_lds", 1)
    ref = eng.cofold_sample_structures(pairs, S, seeds)
    assert all(len(s) == 37 for row in ref[0] for s in row)
    eng.set_option("cofold_lds", 0)
    try:
        off = eng.cofold_sample_structures(pairs, S, seeds)
    finally:
        eng.set_option("cofold_lds", 1)
    assert off[0] == ref[0] and (off[1] == ref[1]).all() and (off[2] == ref[2]).all()
    for k in (0, 5, 63):                                                             # R = 1
        one = eng.cofold_sample_structures([pairs[k]], S, seeds[k:k + 1])
        assert one[0][0] == ref[0][k] and (one[1][0] == ref[1][k]).all()
    small = E.Engine(max_R=8, max_L=64, device=0)                                   # chunks of max_R
    try:
        c0 = small.get_option("cofold_sample_calls")
        got = small.cofold_sample_structures(pairs, S, seeds)
        assert small.get_option("cofold_sample_calls") == c0 + MAX_R // 8
    finally:
        small.close()
    assert got[0] == ref[0] and (got[1] == ref[1]).all() and (got[2] == ref[2]).all()
    monkeypatch.setenv("DRNA_WS_GB", "0.1")
    tight = E.Engine(max_R=MAX_R, max_L=400, device=0)                              # chunks of the workspace slots
    try:
        slots = tight.get_option("workspace_slots")
        assert slots < MAX_R // 2, slots
        c0 = tight.get_option("cofold_sample_calls")
        got = tight.cofold_sample_structures(pairs, S, seeds)
        assert tight.get_option("cofold_sample_calls") == c0 + (MAX_R + slots - 1) // slots
    finally:
        tight.close()
    assert got[0] == ref[0] and (got[1] == ref[1]).all() and (got[2] == ref[2]).all()


def test_errors_as_the_ensemble_defect_reports_them(eng, blob):
    from desirna_amd import engine as E
    rng = np.random.default_rng(4)
    good = [ppr.two_strand_case(rng, 18, 18, "ACGU", True) for _ in range(2)]
    bad = good[0][:7] + "X" + good[0][8:]
    eng.set_targets(["." * 36])
    before = eng.cofold_sample_structures(good, 16, seed=1)
    codes = []
    for call in (lambda: eng.cofold_ensemble_defect([good[0], bad, good[1]]), lambda: eng.cofold_sample_structures([good[0], bad, good[1]], 16, seed=1)):
        with pytest.raises(E.EngineError) as ex:
            call()
        assert "sequence 1" in str(ex.value)
        codes.append(ex.value.code)
    assert codes == [ERR_SEQUENCE, ERR_SEQUENCE]
    after = eng.cofold_sample_structures(good, 16, seed=1)              # the neighbours, and the engine, are as before
    assert after[0] == before[0] and (after[1] == before[1]).all()
    # a partition function out of range: stacking energies of -40 kcal/mol
    hot = np.array(blob, dtype=np.int32, copy=True)
    hot[3:3 + 64] = np.where(hot[3:3 + 64] < 0, -4000, hot[3:3 + 64])
    e2 = E.Engine(max_R=4, max_L=32, device=0, params=hot)
    try:
        e2.set_targets(["." * 32])
        trio = ["A" * 16 + "&" + "A" * 16, "G" * 16 + "&" + "C" * 16, "A" * 16 + "&" + "A" * 16]
        codes = []
        for call in (lambda: e2.cofold_ensemble_defect(trio), lambda: e2.cofold_sample_structures(trio, 8)):
            with pytest.raises(E.EngineError) as ex:
                call()
            assert "sequence 1" in str(ex.value)
            codes.append(ex.value.code)
        assert codes == [ERR_PF_RANGE, ERR_PF_RANGE]
        ss, Es, _ = e2.cofold_sample_structures([trio[0], trio[2]], 8)
        assert all(s == "." * 16 + "&" + "." * 16 for row in ss for s in row) and (Es == 0).all()
    finally:
        e2.close()


def test_argument_errors(eng):
    good = "GGGAAACGGAAACCGA"
    seeds = np.zeros(1, dtype=np.uint64)
    buf = np.zeros(16, dtype=np.uint8)
    call = eng._L.drna_cofold_sample_structures_batch
    # R x S x L beyond the documented limit (1 << 30): refused before anything is written
    assert call(eng._h, 1, 16, 8, good.encode(), (1 << 26) + 1, seeds.ctypes.data, buf.ctypes.data, None, None) == ERR_ARG and not buf.any()
    assert call(eng._h, 1, 16, 8, good.encode(), 4, None, buf.ctypes.data, None, None) == ERR_ARG            # no seeds
    assert call(eng._h, 1, 16, 8, good.encode(), 0, seeds.ctypes.data, buf.ctypes.data, None, None) == ERR_ARG   # S < 1
    assert call(eng._h, 1, 16, 0, good.encode(), 1, seeds.ctypes.data, buf.ctypes.data, None, None) == ERR_ARG   # cut < 1
    assert call(eng._h, 1, 16, 16, good.encode(), 1, seeds.ctypes.data, buf.ctypes.data, None, None) == ERR_ARG  # cut = L
    assert not buf.any()
    assert call(eng._h, 1, 16, 8, good.encode(), 1, seeds.ctypes.data, buf.ctypes.data, None, None) == 0         # E and F4 may be NULL
    assert set(bytes(buf).decode()) <= set("().")
