"""The LDS-resident second-best kernels (fold_subopt_lds.hpp: C, M, M2 in shared memory) compiled for the CPU: against the oracle
(the two lowest energies and the reference's -nd on value of one strand; the co-fold MFE of two) and, with ==, against the
emulated general kernels (subopt_kernel / cofold_subopt_kernel), whose own checks are tests/test_kernels_emulated.py and
tests/test_cofold_subopt_emulated.py."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.emu import emu_subopt_lds
from tests.emu.emu_subopt_lds import INF_REF

ST_BAD_CHAR = 1


@pytest.fixture(scope="module")
def emu(blob):
    return emu_subopt_lds.EmuSuboptLds(blob)


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _cases(M):
    """name -> sequence or pair; M = SUB_LDS_MAX"""
    rng = np.random.default_rng(404)
    c = {"n%d" % n: _rand(rng, n) for n in range(1, 41)}               # every n up to 40 (1, 5 and 6 among them)
    c["max"] = _rand(rng, M)
    c["all_A"] = "A" * 20
    c["GC"] = _rand(rng, 24, "GC")
    c["1+1"] = "G&C"
    c["1+(max-1)"] = _rand(rng, 1) + "&" + _rand(rng, M - 1)
    c["(max-1)+1"] = _rand(rng, M - 1) + "&" + _rand(rng, 1)
    c["18+18"] = _rand(rng, 18) + "&" + _rand(rng, 18)
    x = _rand(rng, 12, "GGCCAU")
    c["X&X"] = x + "&" + x
    return c


WG128 = ("n6", "n14", "n23", "1+1", "X&X")        # also with workgroups of 128 threads (two waves: the barriers matter)


@pytest.fixture(scope="module")
def results(emu):
    """every case through the LDS kernel and the general kernel (64 threads), some through the LDS kernel with 128: computed once"""
    cases = _cases(emu.max_len)
    jobs = [(name, lds, 64) for name in cases for lds in (True, False)] + [(name, True, 128) for name in WG128]
    jobs.sort(key=lambda j: -len(cases[j[0]]))                         # the longest first: they decide the wall time
    got = emu_subopt_lds.second_best_many([(cases[name], lds, nt) for name, lds, nt in jobs])
    return cases, dict(zip(jobs, got))


def test_bound_and_layout(emu):
    assert emu.max_len >= 64                        # every pair of the co-fold LDS path
    assert emu.lds_bytes <= 160 * 1024


def test_lds_equals_general_kernel_everywhere(results):
    cases, got = results
    for name in cases:
        assert got[(name, True, 64)] == got[(name, False, 64)], name
        assert got[(name, True, 64)][2] == 0, name
    for name in WG128:
        assert got[(name, True, 128)] == got[(name, True, 64)], name


def test_one_strand_against_the_oracle(results, oracle):
    cases, got = results
    for name, s in cases.items():
        if "&" in s:
            continue
        e2, e12, st = got[(name, True, 64)]
        assert e12 == oracle.two_best(s), name
        assert e2 == oracle.subopt_energy(s), name
        assert e12[0] == oracle.mfe(s)[1], name


def test_two_strands_against_the_oracle(results, oracle):
    cases, got = results
    for name, s in cases.items():
        if "&" not in s:
            continue
        e2, e12, st = got[(name, True, 64)]
        assert e12[0] == oracle.cofold_mfe(s)[1], name
        assert e12[0] <= e12[1] and e2 == (e12[1] if e12[1] < INF_REF and e12[1] - e12[0] <= 4900 else 0), name
    assert got[("1+1", True, 64)][1][1] < INF_REF          # G&C: the open pair and the joined one


def test_one_structure_only(results):
    cases, got = results
    assert got[("all_A", True, 64)] == (0, (0, INF_REF), 0)


def test_second_structure_beyond_the_band(blob):
    """No sequence has its second structure 49 kcal/mol above the first under Turner 1999 (opening one pair costs a few), so the
    band rule runs on a parameter set whose hairpins of four cost 55 kcal/mol: GAAAAC then has the open chain and one hairpin"""
    b = np.array(blob, dtype=np.int32)
    hairpin = 3 + 64 + 6 * 200 + 2 * 40 + 1600 + 8000 + 40000          # params.py: offset of hairpin[31]
    assert b[hairpin + 3] > 0 and b[hairpin + 4] > 0 and b[hairpin + 30] > b[hairpin + 4]      # (the section is where it should be)
    b[hairpin + 4] = 5500
    emu2 = emu_subopt_lds.EmuSuboptLds(b)
    orc = pyoracle.Oracle(b)
    for s in ("GAAAAC", "A&GAAAAC"):
        E2, E12, st = emu2.second_best([s])
        flat = s.split("&")[-1]
        assert not st.any()
        assert tuple(int(x) for x in E12[0]) == orc.two_best(flat) and orc.subopt_energy(flat) == 0
        assert E12[0, 0] == 0 and 4900 < E12[0, 1] < INF_REF and int(E2[0]) == 0
        G2, G12, gst = emu2.second_best([s], lds=False)
        assert (int(G2[0]), list(G12[0]), int(gst[0])) == (int(E2[0]), list(E12[0]), int(st[0]))


@pytest.mark.parametrize("seqs", [["GGGAAACCCA", "GGGANACCCA", "GCGAAAGCAU"], ["GGGAAC&GUUCCC", "GGGXAC&GUUCCC", "GCGCAU&AUGCGC"]])
def test_bad_letter_inside_a_batch(emu, seqs):
    E2, E12, st = emu.second_best(seqs)
    G2, G12, gst = emu.second_best(seqs, lds=False)
    assert list(st) == [0, ST_BAD_CHAR, 0] and int(E2[1]) == 0
    assert list(E2) == list(G2) and E12.tolist() == G12.tolist() and list(st) == list(gst)
    for k in (0, 2):                                                  # the neighbours of the bad one: the single-sequence values
        one = emu.second_best([seqs[k]])
        assert (int(one[0][0]), one[1][0].tolist()) == (int(E2[k]), E12[k].tolist())
