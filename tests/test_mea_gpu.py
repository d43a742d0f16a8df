"""MEA and centroid structures on the GPU (Engine.mea_structures / cofold_mea_structures: the inside and outside pass of the
ensemble defect, then mea_kernel<512> on the pair probabilities they leave on the device).  Every check is made against the
RETURNED matrix, which the ensemble-defect tests pin: the value against the numpy recurrence of tests/mea_ref.py (no pruning)
within the derived tolerance, the string well-formed and of that value, the centroid exact, the energies those of score_batch /
cofold_batch on the same strings; one strand also against the recurrence on the ORACLE's matrix within the project's 1e-10 per
entry.  Lengths: 1, 5, 12, 36, 40 | 41 (the fused inside + outside launch ends), mea_lds_max | + 1 (M leaves LDS), 260."""
import csv
import subprocess
import sys

import numpy as np
import pytest

from tests import mea_ref as mr
from tests import pair_prob_ref as ppr

pytestmark = pytest.mark.gpu

GAMMAS = (0.25, 1.0, 4.0)
ERR_ARG, ERR_SEQUENCE = -1, -4
HAIRPIN = "GGGCGCGAAAGCGCCC"
PAIR_SHAPES = [(5, 5), (30, 27), (30, 28), (40, 60)]


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=16, max_L=264, device=0)
    yield e
    e.close()


def one_strand_cases(eterna_solutions, lds_max):
    rng = np.random.default_rng(11)
    cases = ["G", "GAAAC"] + [s for s, _ in mr.eterna_by_length(eterna_solutions, (12, 36, 40))]
    cases += [ppr.rand_seq(rng, 41)]
    cases += [ppr.two_strand_case(rng, lds_max // 2, lds_max - lds_max // 2, "ACGU", True).replace("&", "")]
    cases += [ppr.two_strand_case(rng, lds_max // 2, lds_max + 1 - lds_max // 2, "ACGU", True).replace("&", "")]
    cases += ["AAAA".join([HAIRPIN] * 13) + "AAAA"]   # 260 nt, thirteen strong hairpins: a sparse matrix
    return cases


def check_against_returned(P, out, k, g):
    """value, string and centroid of sequence k against the matrix the call returned"""
    n = P.shape[0] - 1
    db, val = out["mea"][k], float(out["mea_value"][k])
    _, want = mr.mea(P, g)
    print("n = %d gamma = %g: value %.17g, recurrence %.17g, tol %.3g" % (n, g, val, want, mr.tol(n, g)))
    assert abs(val - want) <= mr.tol(n, g)
    assert mr.well_formed(P, db) and abs(mr.expected_accuracy(P, db, g) - val) <= mr.tol(n, g)
    cen, dist = mr.centroid(P)
    assert out["centroid"][k].replace("&", "") == cen and abs(float(out["centroid_distance"][k]) - dist) <= mr.tol(n, g)


ONE_STRAND = [1, 5, 12, 36, 40, 41, "mea_lds_max", "mea_lds_max + 1", 260]


@pytest.mark.parametrize("k", range(len(ONE_STRAND)), ids=[str(x) for x in ONE_STRAND])
def test_one_strand(eng, oracle, eterna_solutions, k):
    lds_max = eng.get_option("mea_lds_max")
    cases = one_strand_cases(eterna_solutions, lds_max)
    assert [len(s) for s in cases] == [1, 5, 12, 36, 40, 41, lds_max, lds_max + 1, 260]
    assert eng.get_option("edef_lds_max") == 40
    seq = cases[k]
    n = len(seq)
    _, P_orc = oracle.ensemble_defect(seq, "." * n, want_bpp=True)
    for g in GAMMAS:
        c0 = eng.get_option("mea_calls")
        out = eng.mea_structures([seq], g, want_bpp=True)
        assert eng.get_option("mea_calls") == c0 + 1
        P = out["bpp"][0]
        check_against_returned(P, out, 0, g)
        _, v_orc = mr.mea(P_orc, g)
        assert abs(float(out["mea_value"][0]) - v_orc) <= n * n * 1e-10 * (1 + 2 * g), (n, g)
        if n >= 5:
            eng.set_targets([out["mea"][0], out["centroid"][0]])
            assert (eng.score_batch([seq])["Ed"][0] == out["E"][0]).all()
        else:
            assert (out["E"] == 0).all()
    if n == 260:
        assert eng.get_option("mea_candidates") < 4 * n              # the pruning leaves about one candidate per paired column
    t = eng.last_mea_timing()
    assert t["inside"] > 0 and t["mea"] > 0


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "%d+%d" % s)
def test_two_strands(eng, shape):
    assert eng.get_option("cofold_edef_lds_max") == 57
    pair = ppr.two_strand_case(np.random.default_rng(300 + shape[0]), shape[0], shape[1], "ACGU", True)
    flat, cut = ppr.split(pair)
    for g in GAMMAS:
        out = eng.cofold_mea_structures([pair], g, want_bpp=True)
        P = out["bpp"][0]
        eng.set_targets(["." * len(flat)])
        _, P_edef = eng.cofold_ensemble_defect([pair], want_bpp=True)
        assert P.tobytes() == P_edef[0].tobytes()                         # the matrix of the ensemble defect, same bits
        assert out["mea"][0][cut] == "&" and out["centroid"][0][cut] == "&"
        check_against_returned(P, out, 0, g)
        eng.set_targets([out["mea"][0].replace("&", ""), out["centroid"][0].replace("&", "")])
        assert (eng.cofold_batch([pair])["Ed"][0] == out["E"][0]).all()
    if shape != (5, 5):
        assert any(i <= cut < j for i, j in ppr.pairs_of(out["mea"][0]))  # the planted duplex: a structure across the nick


def test_lds_and_workspace_forms_are_bit_identical(eng, eterna_solutions):
    seqs = [s for s, _ in mr.eterna_by_length(eterna_solutions, (36, 80))] + [ppr.rand_seq(np.random.default_rng(5), 146)]
    assert eng.get_option("mea_lds") == 1
    for seq in seqs:
        a = eng.mea_structures([seq], 1.0, want_bpp=True)
        eng.set_option("mea_lds", 0)
        b = eng.mea_structures([seq], 1.0, want_bpp=True)
        eng.set_option("mea_lds", 1)
        assert a["bpp"].tobytes() == b["bpp"].tobytes()
        assert a["mea"] == b["mea"] and a["centroid"] == b["centroid"] and (a["E"] == b["E"]).all()
        assert a["mea_value"].tobytes() == b["mea_value"].tobytes()
        assert a["centroid_distance"].tobytes() == b["centroid_distance"].tobytes()


def test_chunks_equal_the_sequences_alone():
    from desirna_amd import engine
    e = engine.Engine(max_R=4, max_L=64, device=0)
    try:
        rng = np.random.default_rng(21)
        seqs = [ppr.two_strand_case(rng, 22, 22, "ACGU", True).replace("&", "") for _ in range(9)]
        c0 = e.get_option("mea_calls")
        out = e.mea_structures(seqs, 1.0, want_bpp=True)
        assert e.get_option("mea_calls") == c0 + 3                           # 9 sequences, 4 at a time
        for k, s in enumerate(seqs):
            one = e.mea_structures([s], 1.0, want_bpp=True)
            assert one["bpp"][0].tobytes() == out["bpp"][k].tobytes()
            assert one["mea"][0] == out["mea"][k] and one["centroid"][0] == out["centroid"][k]
            assert one["mea_value"][0] == out["mea_value"][k] and one["centroid_distance"][0] == out["centroid_distance"][k]
            assert (one["E"][0] == out["E"][k]).all()
        assert len(set(out["mea"])) > 1
    finally:
        e.close()


def test_all_a_sequence(eng):
    out = eng.mea_structures(["A" * 30], 1.0, want_bpp=True)
    assert not out["bpp"].any()
    assert out["mea"] == ["." * 30] and out["centroid"] == ["." * 30]
    assert out["mea_value"][0] == 30.0 and out["centroid_distance"][0] == 0.0 and (out["E"] == 0).all()


def test_error_codes_and_installed_targets(eng):
    from desirna_amd.engine import EngineError
    good = "GGGAAAUCCGCGAAAGCAAAACC"
    target = "(((...))).............."
    eng.set_targets([target])
    ed0, bpp0 = eng.ensemble_defect([good], want_bpp=True)
    Ed0 = eng.score_batch([good])["Ed"].copy()
    out = eng.mea_structures([good], 1.0, want_bpp=True)
    assert out["bpp"].tobytes() == bpp0.tobytes()                             # the matrix of the ensemble defect, same bits
    with pytest.raises(EngineError) as ex:
        eng.mea_structures([good, good[:7] + "X" + good[8:], good], 1.0)
    assert ex.value.code == ERR_SEQUENCE and "sequence 1" in str(ex.value)
    for g in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(EngineError) as ex:
            eng.mea_structures([good], g)
        assert ex.value.code == ERR_ARG
    with pytest.raises(EngineError) as ex:
        eng.cofold_mea_structures(["GGGAAA&UUUCCC"], 0.0)
    assert ex.value.code == ERR_ARG
    buf = np.zeros(64, dtype=np.uint8)
    val = np.zeros(1)
    rc = eng._L.drna_mea_structures_batch(eng._h, 1, len(good), good.encode(), 1.0, buf.ctypes.data, val.ctypes.data, None,
                                          val.ctypes.data, None, None)
    assert rc == ERR_ARG and not buf.any()
    # the installed targets are what they were
    ed1 = eng.ensemble_defect([good])
    assert ed1.tobytes() == ed0.tobytes() and (eng.score_batch([good])["Ed"] == Ed0).all()
    again = eng.mea_structures([good], 1.0)
    assert again["mea"] == out["mea"] and again["mea_value"][0] == out["mea_value"][0]


def test_needs_no_targets():
    from desirna_amd import engine
    e = engine.Engine(max_R=2, max_L=30, device=0)
    try:
        out = e.mea_structures(["GGGGAAAACCCC"], 1.0)
        assert out["mea"] == ["((((....))))"] and out["centroid"] == ["((((....))))"]
        out = e.cofold_mea_structures(["GGGG&CCCC"], 1.0)
        assert out["mea"] == ["((((&))))"]
    finally:
        e.close()


def test_cli_run_with_structures(tmp_path):
    """one run of the command line in a fresh process: <name>_structures.csv beside _results.csv for a 24-nt hairpin"""
    from desirna_amd import outputs
    target = "((((((((......)))))))).."
    f = tmp_path / "hp.txt"
    f.write_text(">name\nhp\n>seq_restr\n%s\n>sec_struct\n%s\n" % ("N" * len(target), target))
    out = tmp_path / "out"
    subprocess.run([sys.executable, "-m", "desirna_amd.design", "-f", str(f), "-R", "4", "-s", "2", "--structures", "1.0",
                    "-o", str(out)], check=True, timeout=300)
    (res_file,) = [p for p in out.iterdir() if p.name.endswith("_results.csv")]
    (st_file,) = [p for p in out.iterdir() if p.name.endswith("_structures.csv")]
    reported = [r["sequence"] for r in csv.DictReader(open(res_file))]
    rows = list(csv.DictReader(open(st_file)))
    assert tuple(rows[0].keys()) == outputs.STRUCTURE_COLUMNS
    assert [r["sequence"] for r in rows if r["kind"] == "mfe"] == reported
    for seq in reported:
        mine = [r for r in rows if r["sequence"] == seq]
        assert [r["kind"] for r in mine] == ["mfe", "centroid", "mea"]
        assert all(len(r["structure"]) == len(target) and 0.0 <= float(r["p_structure"]) <= 1.0 + 1e-9 for r in mine)
        assert mine[0]["value"] == "" and float(mine[1]["value"]) >= 0.0 and float(mine[2]["value"]) > 0.0
