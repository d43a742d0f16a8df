"""The short-pair co-fold kernels (fold_cofold_lds.hpp: every table in LDS) compiled for the CPU and checked against the oracle:
structures and Emfe exact, the four free energies within 1e-9 kcal/mol (summation-order differences only)."""
import numpy as np
import pytest

from tests.emu import emu_cofold_lds

F4_TOL = 1e-9
ST_BAD_CHAR = 1


@pytest.fixture(scope="module")
def emu(blob):
    return emu_cofold_lds.EmuCofoldLds(blob)


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _check(emu, oracle, seqs, nt):
    E, ss, F4, st = emu.cofold(seqs, nt=nt)
    assert not st.any()
    for k, s in enumerate(seqs):
        assert (ss[k], int(E[k])) == oracle.cofold_mfe(s), s
        assert max(abs(g - o) for g, o in zip(F4[k], oracle.cofold_pf(s))) < F4_TOL, s


@pytest.mark.parametrize("nt", [64, 128])
def test_random_pairs_against_the_oracle(emu, oracle, nt):
    """(the emulation's cost is its barriers, which grow with the workgroup: the longest pairs run with 64 threads only)"""
    rng = np.random.default_rng(11 + nt)
    M = emu.max_len
    assert M >= 64
    for la, lb in ((1, 1), (2, 5), (17, 18), (25, 11)) + (((1, M - 1),) if nt == 64 else ()):
        _check(emu, oracle, [_rand(rng, la) + "&" + _rand(rng, lb)], nt)


def test_both_cuts_at_the_longest_pair(emu, oracle):
    rng = np.random.default_rng(5)
    M = emu.max_len
    a = _rand(rng, M // 2)
    _check(emu, oracle, [_rand(rng, M - 1) + "&" + _rand(rng, 1)], 64)
    _check(emu, oracle, [a + "&" + a], 64)                          # two equal strands: the symmetry factor


def test_special_pairs(emu, oracle):
    rng = np.random.default_rng(6)
    _check(emu, oracle, [_rand(rng, 14, "GC") + "&" + _rand(rng, 12, "GC")], 128)
    _check(emu, oracle, ["A" * 9 + "&" + "A" * 7], 64)              # cannot pair at all
    a = _rand(rng, 10)
    _check(emu, oracle, [a + "&" + a], 64)


def test_bad_letter_sets_that_pair_only(emu, oracle):
    seqs = ["GGGAAACC&GGUUUCCC", "GGGANACC&GGUUUCCC", "GCGAAACC&GGUUUCGC"]
    E, ss, F4, st = emu.cofold(seqs, nt=64)
    assert list(st) == [0, ST_BAD_CHAR, 0, 0, ST_BAD_CHAR, 0]
    assert int(E[1]) == 0 and set(ss[1]) == set(".&") and not F4[1].any()
    for k in (0, 2):
        assert (ss[k], int(E[k])) == oracle.cofold_mfe(seqs[k])
        assert max(abs(g - o) for g, o in zip(F4[k], oracle.cofold_pf(seqs[k]))) < F4_TOL
