"""CPU check of the K-best co-fold kernel (cofold_kbest_kernel, desirna_amd/csrc/fold_cofold_subopt.hpp), compiled unmodified
against the HIP stand-in of tests/emu/ into a library of its own.  The reference pins no ranked structure for two strands, so
the kernel is checked against explicit enumeration of every co-fold structure, each scored by the oracle's two-strand
evaluation.  The order among structures of equal energy is the engine's own: energies are compared as sorted lists, strings by
membership, re-evaluation and distinctness.  Last, ``outputs.get_alt_mcc`` on two-strand records over the emulated call."""
import numpy as np
import pytest

from tests import cofold_kbest_cases as cases
from tests import constructs as C
from tests.emu.emu import cofold_subopt_many
from tests.emu.emu_cofold_kbest import INF_REF, cofold_kbest, cofold_kbest_many
from tests.test_cofold_subopt_emulated import _enumeration_cases, _rand, cofold_structures, rotate

ST_BAD_CHAR = 1


def _flat(s):
    return s.replace("&", ""), s.index("&")


def _check_strings(oracle, s, E, ss, members=None):
    """what holds for every answer: ascending energies, finite ranks first; each finite string is a structure of the pair
    (a member of the enumerated set where there is one), has the energy reported for it and the '&' at the cut; the finite
    strings are pairwise different; all dots beyond"""
    flat, cut = _flat(s)
    E = [int(e) for e in E]
    assert E == sorted(E), (s, E)
    fin = [x for e, x in zip(E, ss) if e < INF_REF]
    assert len(set(fin)) == len(fin), (s, fin)
    for e, x in zip(E, ss):
        assert len(x) == len(s) and x[cut] == "&", (s, x)
        db = x.replace("&", "")
        if e < INF_REF:
            assert members is None or db in members, (s, x)
            assert db.count("(") == db.count(")")
            assert oracle.eval_structure(flat, db, cut) == e, (s, x, e)
        else:
            assert db == "." * len(flat), (s, x)


@pytest.fixture(scope="module")
def enumerated(oracle):
    """the 60 enumeration cases: per case the set of structures and their sorted energies"""
    out = []
    for s in _enumeration_cases():
        flat, cut = _flat(s)
        dbs = cofold_structures(flat, cut)
        out.append((s, set(dbs), sorted(oracle.eval_structure(flat, db, cut) for db in dbs)))
    return out


@pytest.fixture(scope="module")
def kbest_runs(enumerated):
    """every enumeration case at K = 4 and 8 in workgroups of 64 and 128: {(K, nt): [(E, strings, status), ...]}"""
    keys = [(K, nt) for K in (4, 8) for nt in (64, 128)]
    got = cofold_kbest_many([(s, K, nt) for K, nt in keys for s, _, _ in enumerated])
    n = len(enumerated)
    return {key: got[k * n:(k + 1) * n] for k, key in enumerate(keys)}


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("nt", [64, 128])
def test_against_enumeration(oracle, enumerated, kbest_runs, K, nt):
    for (s, members, en), (E, ss, st) in zip(enumerated, kbest_runs[(K, nt)]):
        assert st == 0, s
        assert E == (en + [INF_REF] * K)[:K], (s, K, nt)
        _check_strings(oracle, s, E, ss, members)


def test_record_for_the_gpu_test_is_current(oracle, enumerated, kbest_runs):
    """tests/golden/cofold_kbest_emulated.json, which tests/test_cofold_kbest_gpu.py compares the GPU with byte for byte, is what
    the emulated kernel gives now: the enumeration pairs from the runs above, the longer pairs emulated here"""
    seqs, rec = cases.load()
    assert seqs == cases.pairs()
    n = len(enumerated)
    assert seqs[:n] == [s for s, _, _ in enumerated]
    fresh = cases.emulate(seqs[n:])
    for K in cases.KS:
        assert rec[K][:n] == [[E, ss] for E, ss, st in kbest_runs[(K, cases.NT)]], K
        assert rec[K][n:] == fresh[K], K
        for s, (E, ss) in zip(seqs[n:], rec[K][n:]):
            assert E[0] == oracle.cofold_mfe(s)[1], s
            _check_strings(oracle, s, E, ss)


def test_rank0_and_rank1(oracle, enumerated, kbest_runs):
    """rank 0 is the co-fold MFE, ranks 0 and 1 are what the second-best kernel reports"""
    e12 = cofold_subopt_many([s for s, _, _ in enumerated])
    for (s, _, _), (E, ss, st), (_, two, st2) in zip(enumerated, kbest_runs[(8, 128)], e12):
        assert st == 0 and st2 == 0
        assert E[0] == oracle.cofold_mfe(s)[1], s
        assert tuple(E[:2]) == tuple(two), s


def test_fewer_than_k_structures(oracle):
    """one, two and three structures: the list ends in INF_REF / all dots exactly where the enumeration ends"""
    cases = [("AAAA&AAAA", 1), ("AG&CA", 2), ("G&C", 2), ("GG&C", 3)]
    got = cofold_kbest_many([(s, K, 64) for s, _ in cases for K in (4, 8)])
    for k, (s, count) in enumerate(cases):
        flat, cut = _flat(s)
        dbs = cofold_structures(flat, cut)
        assert len(dbs) == count, (s, dbs)
        en = sorted(oracle.eval_structure(flat, db, cut) for db in dbs)
        for K, (E, ss, st) in zip((4, 8), got[2 * k:2 * k + 2]):
            assert st == 0
            assert E == en + [INF_REF] * (K - count), (s, E)
            assert sum(e < INF_REF for e in E) == count
            _check_strings(oracle, s, E, ss, set(dbs))


def test_unconnected_only_pairs(oracle):
    """nothing can join {G, C} to A: no returned string has a pair across the cut, and the energies are those of the G/C
    strand alone (no DuplexInit, every structure counted once)"""
    rng = np.random.default_rng(5)
    strands = [_rand(rng, la, "GC") for la in (9, 11, 13, 14)]
    cases = [x + "&" + "A" * lb for x, lb in zip(strands, (6, 4, 9, 12))]
    cases += ["A" * lb + "&" + x for x, lb in zip(strands, (5, 8, 4, 10))]       # mirrored
    K = 8
    got = cofold_kbest_many([(s, K, 128) for s in cases])
    for s, (E, ss, st) in zip(cases, got):
        assert st == 0, s
        x = s.replace("&", "").strip("A") if s[0] == "A" else s.split("&")[0]
        en = sorted(oracle.eval_structure(x, db) for db in cofold_structures(x, len(x)))     # cut at the end: one strand
        assert E == (en + [INF_REF] * K)[:K], s
        _check_strings(oracle, s, E, ss)
        for db in ss:
            a, b = db.split("&")
            assert a.count("(") == a.count(")") and b.count("(") == b.count(")"), (s, db)


def test_homodimer_rotation(oracle):
    """X&X: rotation by one strand maps structures to structures of equal energy, and nothing is reduced by symmetry.  So a
    ground level that the K ranks hold completely is closed under rotation, and where the ground state is not its own rotation
    and has one twin only, ranks 0 and 1 have equal energy and are each other's rotation.  (A level may hold more: the strand
    GGGGUGCCGC has a symmetric ground state and two more of the same energy with one more pair, rotations of each other.)"""
    rng = np.random.default_rng(17)
    xs = []
    while len(xs) < 6:                          # strands whose co-fold ground state is not its own rotation (the oracle picks)
        x = _rand(rng, int(rng.integers(8, 13)), "GGCCAU")
        db = oracle.cofold_mfe(x + "&" + x)[0].replace("&", "")
        if rotate(db, len(x)) != db:
            xs.append(x)
    seqs = [x + "&" + x for x in xs]
    K, twins = 8, 0
    for s, x, (E, ss, st) in zip(seqs, xs, cofold_kbest_many([(s, K, 128) for s in seqs])):
        assert st == 0, s
        g, e = oracle.cofold_mfe(s)
        assert E[0] == E[1] == e, s                                    # the ground state and its twin
        _check_strings(oracle, s, E, ss)
        level = [x1.replace("&", "") for e1, x1 in zip(E, ss) if e1 == e]
        assert len(level) < K, (s, E)                                  # the ranks hold the whole ground level
        assert {rotate(db, len(x)) for db in level} == set(level), (s, level)
        assert g.replace("&", "") in level, (s, g, level)
        if len(level) == 2:
            twins += 1
            assert level[0] != level[1] and rotate(level[0], len(x)) == level[1] and rotate(level[1], len(x)) == level[0], (s, level)
    assert twins >= 3                                                 # (most ground levels are one structure and its twin)


def _constructed_pairs():
    hp = "GCGCGAAAGCGC"
    pairs = [
        # a nick loop with an inner helix on both strands: GGCG ... CGCC joins the strands, a hairpin hangs on either side of the nick
        "GGCG" + "A" + hp + "AA" + "&" + "AA" + hp + "A" + "CGCC",
        # a multiloop whose branch helix encloses the nick: GGCGC ... GCGCC closes it, branches: a hairpin on the first strand
        # and the helix GGCCG & CGGCC that ends at the nick
        "GGCGC" + "A" + hp + "A" + "GGCCG" + "&" + "CGGCC" + "A" + "GCGCC",
        # the two-strand interior forms and the nick inside an interior loop's run
        C.cofold_record(0, 0).sequence, C.cofold_record(2, 1).sequence, C.cofold_record(1, 3).sequence,
        C.nicked_record(1, 1).sequence, C.nicked_record(4, 4).sequence, C.nicked_record(2, 0).sequence,
        # 1 + n and n + 1
        "G" + "&" + "CGCGAAAGCGC", "GCGCGAAAGCG" + "&" + "C", "A" + "&" + hp, hp + "&" + "A",
    ]
    return pairs


def test_constructed_loop_shapes(oracle):
    pairs = _constructed_pairs()
    got = cofold_kbest_many([(s, 8 if k % 2 else 4, 128) for k, s in enumerate(pairs)])
    for s, (E, ss, st) in zip(pairs, got):
        assert st == 0, s
        oss, oe = oracle.cofold_mfe(s)
        assert E[0] == oe, (s, E, oss)
        _check_strings(oracle, s, E, ss)
    # the shapes are there: the first two ground states hold a pair across the nick that closes the nick loop / encloses it
    for s, (E, ss, st) in zip(pairs[:2], got[:2]):
        cut = s.index("&")
        pt = C.pair_table(ss[0])
        assert pt[0] == len(s) - 2, (s, ss[0])                                   # the outermost pair joins the strands
        inner = [(i, j) for i, j in enumerate(pt) if j > i and i > 0]
        assert any(j < cut for i, j in inner), (s, ss[0])                        # a helix inside the first strand
    assert any(i < pairs[1].index("&") <= j and i > 0 for i, j in enumerate(C.pair_table(got[1][1][0]))), got[1][1][0]


def test_batch_and_bad_letter():
    """several pairs in one launch (workspace slots side by side) give the single-pair values; a bad letter is ST_BAD_CHAR
    and INF_REF for that pair only"""
    seqs = ["GGGAAC&GUUCCC", "GCGCAU&AUGCGC", "GGGXAC&GUUCCC", "GGCAUC&GAUGCC"]
    for K in (3, 8):
        E, ss, st = cofold_kbest(seqs, K, nt=64)
        assert list(st) == [0, 0, ST_BAD_CHAR, 0]
        assert [int(e) for e in E[2]] == [INF_REF] * K and ss[2] == ["......&......"] * K
        single = cofold_kbest_many([(s, K, 64) for s in seqs[:2] + seqs[3:]])
        for k, (e1, s1, st1) in zip((0, 1, 3), single):
            assert st1 == 0 and [int(e) for e in E[k]] == e1 and ss[k] == s1, (K, seqs[k])


class _StandInEngine:
    """outputs.get_alt_mcc's engine: two-strand ranked structures from the emulated kernel, the one-strand call must not be taken"""

    def __init__(self):
        self.calls = []

    def cofold_subopt_structs(self, seqs, K):
        self.calls.append((list(seqs), K))
        E, ss, st = cofold_kbest(list(seqs), K, nt=64)
        assert not st.any()
        return E, ss

    def subopt_structs(self, seqs, K):
        raise AssertionError("two-strand records must not take the one-strand call")


def test_get_alt_mcc_two_strands(oracle):
    from desirna_amd import outputs
    alt = "(((.&.)))"
    recs = [{"sequence": s} for s in ("GGGA&UCCC", "AAAA&AAAA", "GCGA&UCGC", "GGCA&UGCC")]
    eng = _StandInEngine()
    out = outputs.get_alt_mcc(recs, [alt], eng)
    assert eng.calls == [([d["sequence"] for d in recs], 2)]           # one call for the one (length, cut), K = #alternatives + 1
    for d in out:
        s = d["sequence"]
        E, ss, st = cofold_kbest([s], 2, nt=64)
        assert set(d) == {"sequence", "mcc_1", "alt_struct_1"}
        assert len(d["alt_struct_1"]) == len(s)
        if int(E[0, 1]) < INF_REF and int(E[0, 1]) - int(E[0, 0]) <= 4900:
            assert d["alt_struct_1"] == ss[0][1] and d["alt_struct_1"][s.index("&")] == "&"
            flat, cut = _flat(s)
            assert oracle.eval_structure(flat, d["alt_struct_1"].replace("&", ""), cut) == int(E[0, 1])
        else:
            assert d["alt_struct_1"] == "." * len(s)                    # the reference's fallback: dots over the '&' column too
        assert 0.0 <= d["mcc_1"] <= 2.0
    assert out[1]["alt_struct_1"] == "." * 9                            # AAAA&AAAA has one structure only
    assert out[0]["alt_struct_1"] != "." * 9
    # rank 1 equal to the alternative target scores 1 - MCC = 0
    hit = [d for d in out if d["alt_struct_1"] == alt]
    assert all(d["mcc_1"] == 0.0 for d in hit)
    with pytest.raises(ValueError):
        outputs.get_alt_mcc([{"sequence": "GGGA&UCCC"}, {"sequence": "GGGAAUCCC"}], [alt], eng)
