"""An exact reference for EVERY rank of the ranked-structure folds, one and two strands (CPU part).

    orc_enum_kbest      (oracle.c) walks every structure and scores it with eval_structure: the root of trust.  Held here to the
                        Python enumerators the older tests use.
    orc_kbest_energies  (oracle.c) the plain serial K-list fill: held here to the enumerator on dense sequences of 18 - 30 nt,
                        pairs up to 14+14 and SPARSE sequences of 100 - 260 nt (tests/kbest_ref.py), under Turner-1999 and the
                        probe parameter sets.
    the emulated kernels (kbest_kernel, cofold_kbest_kernel, the four second-best kernels) are then held to the fill, and to the
                        enumeration where it ran, by the one rule kbest_ref.check_ranked.

Every enumerated case asserts count_structures(case) <= CAP first; nothing is skipped."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import kbest_ref as KR
from tests.probe_params import probe_blob

INF_REF = KR.INF_REF
PARAM_SETS = ("turner1999", "distinct", "distinct_sharp")


@pytest.fixture(scope="module")
def oracles():
    from oracle import pyoracle
    pyoracle.build()
    return {name: pyoracle.Oracle(probe_blob(name)) for name in PARAM_SETS}


def _enumerate(O, s):
    """(energies, strings, count) of the 8 best by enumeration; the size of the case is asserted BEFORE it is walked"""
    c = O.count_structures(s)
    assert c <= KR.CAP, (s, c)
    E, ss, cnt = O.enum_kbest(s, 8)
    assert cnt == c, (s, cnt, c)
    return E, ss, cnt


GROUPS = {
    "dense_one": lambda: KR.dense_one_strand(),
    "dense_two": lambda: KR.dense_two_strands(),
    "sparse_one": lambda: list(KR.sparse_one_strand().values()),
    "sparse_two": lambda: list(KR.sparse_two_strands().values()),
}
_enum_cache = {}


def enumerated(oracles, pname, group):
    """{sequence: (E, ss, count)} of a group under a parameter set, computed once (the oracle calls release the GIL)"""
    key = (pname, group)
    if key not in _enum_cache:
        seqs = GROUPS[group]()
        with ThreadPoolExecutor(8) as ex:
            _enum_cache[key] = dict(zip(seqs, ex.map(lambda s: _enumerate(oracles[pname], s), seqs)))
    return _enum_cache[key]


# ---------------------------------------------------------------------------------------------- enumerator vs Python enumerators

def test_enumerator_against_python_enumerators_one_strand(oracle):
    from tests.test_kernels_emulated import _all_structures, _rand
    rng = np.random.default_rng(77)                 # the cases of test_kbest_structures_against_enumeration
    cases = [_rand(rng, 13), _rand(rng, 15, "GC"), _rand(rng, 14, "GCAU"), "GGGAAACCCA", "AAAAAAAA"]
    rng = np.random.default_rng([KR.SEED, 8])
    cases += [_rand(rng, L, a) for L, a in ((16, "ACGU"), (17, "GC"), (18, "GGCCAU"), (5, "GC"), (1, "A"))]
    for s in cases:
        every = sorted((oracle.eval_structure(s, x), x) for x in _all_structures(s))
        E, ss, cnt = oracle.enum_kbest(s, 8)
        assert cnt == len(every) == oracle.count_structures(s), s
        assert E == ([e for e, _ in every] + [INF_REF] * 8)[:8], s
        assert ss[:min(8, cnt)] == [x for _, x in every[:8]], s                  # ties by string
        assert all(x == "." * len(s) for x in ss[cnt:]), s


def test_enumerator_against_python_enumerators_two_strands(oracle):
    from tests.test_cofold_subopt_emulated import _enumeration_cases, cofold_structures
    for s in _enumeration_cases() + ["G&C", "A&A", "GGGG&CCCC"]:
        cut, flat = s.index("&"), s.replace("&", "")
        every = sorted((oracle.eval_structure(flat, x, cut), x) for x in cofold_structures(flat, cut))
        E, ss, cnt = oracle.enum_kbest(s, 8)
        assert cnt == len(every) == oracle.count_structures(s), s
        assert E == ([e for e, _ in every] + [INF_REF] * 8)[:8], s
        assert ss[:min(8, cnt)] == [x for _, x in every[:8]], s


# ---------------------------------------------------------------------------------------------- oracle fill vs enumeration

@pytest.mark.parametrize("pname,group", [(p, g) for g in GROUPS for p in PARAM_SETS if p != "distinct_sharp" or g.endswith("two")])
def test_fill_against_enumeration(oracles, pname, group):
    O = oracles[pname]
    ref = enumerated(oracles, pname, group)
    assert len(ref) >= (35 if group.startswith("dense") else 9)
    for s, (E, ss, cnt) in ref.items():
        got = O.kbest_energies(s, 8)
        assert got == E, (pname, s, got, E)
        for K in range(1, 8):
            assert O.kbest_energies(s, K) == E[:K], (pname, s, K)               # every shorter K is the prefix
        KR.check_ranked(O, s, E, ss, got, ss)                                   # the enumeration satisfies the rule itself


def test_case_lists_are_what_the_design_asks_for():
    one, two = KR.dense_one_strand(), KR.dense_two_strands()
    assert sum(18 <= len(s) <= 30 for s in one) >= 30 and "A" * 12 in one and KR.ONE_STRUCTURE_MORE in one
    shapes = [(s.index("&"), len(s) - 1 - s.index("&")) for s in two]
    assert sum(6 <= a <= 14 and 6 <= b <= 14 for a, b in shapes) >= 30
    assert {(14, 14), (3, 20), (20, 3), (1, 24), (24, 1)} <= set(shapes)
    assert sum(s.split("&")[0] == s.split("&")[1] for s in two) >= 2
    for name, s in list(KR.sparse_one_strand().items()) + list(KR.sparse_two_strands().items()):
        assert "U" not in s and set(s) <= set("ACG&"), name
        if name.startswith("seeded"):
            assert 12 <= sum(ch in "GC" for ch in s) <= 16, name
    assert {len(s) for s in KR.sparse_one_strand().values()} >= {100, 130, 200, 260}
    assert {(s.index("&"), len(s) - 1 - s.index("&")) for s in KR.sparse_two_strands().values()} >= {(50, 50), (100, 100), (30, 170)}


def test_one_structure_more_and_none(oracle):
    assert oracle.count_structures(KR.ONE_STRUCTURE_MORE) == 2 and oracle.count_structures("A" * 12) == 1
    E = oracle.kbest_energies(KR.ONE_STRUCTURE_MORE, 8)
    assert E[0] == 0 and 0 < E[1] < INF_REF and E[2:] == [INF_REF] * 6
    assert oracle.kbest_energies("A" * 12, 8) == [0] + [INF_REF] * 7
    assert oracle.kbest_energies("A&A", 4) == [0] + [INF_REF] * 3


def test_sparse_cases_hold_the_loops_they_were_built_for(oracles):
    """what the eight best of the sparse cases contain (Turner-1999): the point of the long cases"""
    one = KR.sparse_one_strand()
    ref = enumerated(oracles, "turner1999", "sparse_one")
    best = {name: [KR.loops(x) for e, x in zip(ref[s][0], ref[s][1]) if e < INF_REF] for name, s in one.items()}
    flat = lambda name: [l for ls in best[name] for l in ls]
    assert any(k == "H" and size > 30 for name in best for k, size, _, _ in flat(name))            # hairpins longer than 30
    assert any(k == "H" and size >= 70 for k, size, _, _ in flat("hairpin35_200"))
    assert any(k == "I" and size == 30 for k, size, _, _ in best["interior30_100"][0])               # MAXLOOP in the ground state
    assert any(k == "I" and size == 29 for k, size, _, _ in best["interior29_100"][0])
    assert any(k == "I" and size == 30 for k, size, _, _ in best["bulge30_100"][0])
    assert not any(k == "I" and size > 30 for name in best for k, size, _, _ in flat(name))          # nothing above MAXLOOP
    assert not any(k == "I" and size > 8 for k, size, _, _ in flat("interior31_100"))                # 31 cannot form
    for name in ("multiloop3_130", "multiloop3_260"):
        assert any(k == "M" and stems >= 3 and size >= 60 and span > 64 for k, size, stems, span in best[name][0]), name
    two = KR.sparse_two_strands()
    ref2 = enumerated(oracles, "turner1999", "sparse_two")
    for name in ("multiloop3_nick_50+50", "multiloop3_nick_30+170"):
        s = two[name]
        ls = [l for e, x in zip(*ref2[s][:2]) for l in KR.loops(x, s.index("&"))]
        assert any(k == "M" and stems >= 3 for k, _, stems, _ in ls), name
        assert any(k == "N" for k, _, _, _ in ls), name
    s = two["interior30_50+50"]
    assert any(k == "I" and size == 30 for k, size, _, _ in KR.loops(ref2[s][1][0], s.index("&")))


def test_k2_is_two_best(oracle):
    """orc_two_best stays: the K = 2 fill gives its values (and the co-fold MFE for two strands) at working lengths"""
    rng = np.random.default_rng([KR.SEED, 9])
    for s in KR.dense_one_strand() + [KR._rand(rng, L, a) for L in (5, 64, 100, 260) for a in ("ACGU", "GC")]:
        assert tuple(oracle.kbest_energies(s, 2)) == oracle.two_best(s), s
        assert oracle.kbest_energies(s, 1)[0] == oracle.mfe(s)[1], s
    for la, lb in ((18, 18), (1, 35), (40, 17), (100, 100)):
        s = KR._rand(rng, la) + "&" + KR._rand(rng, lb)
        assert oracle.kbest_energies(s, 1)[0] == oracle.cofold_mfe(s)[1], s


def test_the_rule_bites(oracles):
    """check_ranked refuses an answer that lost a rank, repeats a string, or reports a string under a wrong energy"""
    O = oracles["turner1999"]
    ref = enumerated(oracles, "turner1999", "dense_one")
    s = next(s for s in KR.dense_one_strand() if len(set(ref[s][0])) == 8)      # eight different energies: no ties to excuse anything
    E, ss, _ = ref[s]
    KR.check_ranked(O, s, E[:5], ss[:5], E, ss)
    for bad_E, bad_ss in ((E[:2] + E[3:], ss[:2] + ss[3:]),                 # rank 2 dropped
                          (E[:4], ss[:3] + ss[2:3]),                        # a string twice
                          (E[:4], ss[:3] + ss[4:5])):                       # a string of another energy, or a missing structure
        with pytest.raises(AssertionError):
            KR.check_ranked(O, s, bad_E, bad_ss, E, ss)


# ---------------------------------------------------------------------------------------------- emulated kernels vs the fill

# interior30_100 of kbest_ref cut to 72 nt: the two helices and the interior loop of MAXLOOP between them, enumerated below
SPARSE_EMULATED = KR._fill(72, 5, "GGGG", 15, "GGG", 4, "CCC", 15, "CCCC")


def _emu_cases():
    rng = np.random.default_rng([KR.SEED, 10])
    dense30 = next(s for s in KR.dense_one_strand() if len(s) == 30)
    kb = [dense30, KR._rand(rng, 44), SPARSE_EMULATED, KR.NAMED_ONE["multiloop_tail_29"], KR.NAMED_ONE["full_lists_28"],
          next(s for s in KR.dense_two_strands() if s.index("&") == 14 and len(s) == 29), KR._rand(rng, 22) + "&" + KR._rand(rng, 22)]
    kb += list(KR.NAMED_TWO.values())
    sb = [KR._rand(rng, 44), KR._rand(rng, 79, "GGCCAU"), KR._rand(rng, 22) + "&" + KR._rand(rng, 22), KR._rand(rng, 40) + "&" + KR._rand(rng, 39)]
    return kb, sb


def _emu_ks(s):
    """the kernel instances (lists of 4, of 8) an emulated K-best case goes through.  Both: the short cases (30 nt, 14+14, the named
    multiloop and nick cases).  Lists of 4 only: the two sparse cases of 64 - 72 nt.  Lists of 8 only: 44 nt, 22+22 and the cases
    named for full lists of 8.  Emulation time grows steeply with length and doubles with the list size; both instances of both
    kernels meet the sparse 100 - 260 nt cases, enumerated, in tests/test_kbest_reference_gpu.py"""
    if s in (SPARSE_EMULATED, KR.NAMED_TWO["nick_lists_20+44"]):
        return (4,)
    if s in (KR.NAMED_ONE["full_lists_28"], KR.NAMED_TWO["nick_lists_11+12"], KR.NAMED_TWO["nick_lists_11+10"]) or len(s) > 30:
        return (8,)
    return (4, 8)


def _emu_paths(s):
    """lds False / True = the general / the LDS second-best kernel: both at 44 nt and 22+22, the LDS kernel alone at 79 nt and 40+39
    (the general kernels run the same kbest_fill and meet these lengths on the GPU)"""
    return (False, True) if len(s) < 60 else (True,)


@pytest.fixture(scope="module")
def emulated():
    """every emulated run of this module, spread over worker processes once"""
    from tests.emu.emu_cofold_kbest import cofold_kbest_many
    from tests.emu.emu_subopt_lds import second_best_many
    kb, sb = _emu_cases()
    kjobs = [(s, K, 64) for s in kb for K in _emu_ks(s)]
    sjobs = [(s, lds, 64) for s in sb for lds in _emu_paths(s)]
    return dict(zip(kjobs, cofold_kbest_many(kjobs, workers=6))), dict(zip(sjobs, second_best_many(sjobs, workers=6)))


@pytest.mark.parametrize("K", [4, 8])
def test_emulated_kbest_kernels(oracle, oracles, emulated, K):
    """kbest_kernel<64,K> at 30 and 44 nt, two named cases and a sparse 72 nt; cofold_kbest_kernel<64,K> at 14+14, 22+22 and the
    named nick cases, one of them a sparse 20+44"""
    kb, _ = _emu_cases()
    groups = [enumerated(oracles, "turner1999", g) for g in GROUPS]
    for s in kb:
        if K not in _emu_ks(s):
            continue
        E, ss, st = emulated[0][(s, K, 64)]
        assert st == 0, s
        hit = [g[s] for g in groups if s in g] + ([_enumerate(oracle, s)] if s == SPARSE_EMULATED else [])
        ref_E, ref_ss = (hit[0][0], hit[0][1]) if hit else (oracle.kbest_energies(s, 8), None)
        assert ref_E == oracle.kbest_energies(s, 8), s
        KR.check_ranked(oracle, s, E, ss, ref_E, ref_ss)
    assert sum(1 for s in kb if any(s in g for g in groups)) == 8               # all but 44 nt and 22+22 are enumerated (the 72-nt sparse case above)


@pytest.mark.parametrize("lds", [False, True])
def test_emulated_second_best_kernels(oracle, emulated, lds):
    """subopt_kernel / subopt_lds_kernel at 44 and 79 nt, cofold_subopt_kernel / cofold_subopt_lds_kernel at 22+22 and 40+39:
    ranks 0 and 1 and the 4900-dcal rule"""
    _, sb = _emu_cases()
    for s in sb:
        if lds not in _emu_paths(s):
            continue
        e2, e12, st = emulated[1][(s, lds, 64)]
        assert st == 0, s
        want = oracle.kbest_energies(s, 2)
        assert list(e12) == want, (s, lds)
        assert e2 == (want[1] if want[1] < INF_REF and want[1] - want[0] <= 4900 else 0), (s, lds)
