"""The self-dimer partition function kernels (fold_self_dimer.hpp: s & s on ~1.5 L^2 cells, tables in LDS or in a workspace slot)
compiled for the CPU and checked against the oracle's co-fold partition function of s + "&" + s: the four free energies within
1e-9 kcal/mol (summation-order differences only), oligo_fraction by the reference's formula on the oracle's values."""
import numpy as np
import pytest

from desirna_amd import energy_scores as es
from tests.emu import emu_self_dimer

F4_TOL = 1e-9
ST_BAD_CHAR = 1


@pytest.fixture(scope="module")
def emu(blob):
    return emu_self_dimer.EmuSelfDimer(blob)


@pytest.fixture(scope="module")
def pair_emu(blob):
    from tests.emu import emu_cofold_lds
    return emu_cofold_lds.EmuCofoldLds(blob)


def _rand(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(list(alphabet), size=n))


def _frac(F):
    with np.errstate(invalid="ignore"):
        return float(es.oligo_fraction(F[0], F[1], F[2]))


def _check(emu, oracle, seqs, nt, lds=True):
    F4, st = emu.fold(seqs, nt=nt, lds=lds)
    assert not st.any()
    for k, s in enumerate(seqs):
        want = oracle.cofold_pf(s + "&" + s)
        assert max(abs(g - o) for g, o in zip(F4[k], want)) < F4_TOL, (s, list(F4[k]), want)
        # the fraction's own error: d frac / d F <= 1 / kT ~ 1.6 per kcal/mol, three energies of F4_TOL each
        # (a sequence that cannot pair: FcAA = 999, and the reference's formula gives 0 / 0 on both sides)
        fg, fw = _frac(F4[k]), _frac(want)
        assert (np.isnan(fg) and np.isnan(fw)) or abs(fg - fw) < 3 * 1.7 * F4_TOL, s
    return F4


@pytest.mark.parametrize("nt,lds", [(64, True), (128, True), (64, False)])
def test_smallest_lengths_at_which_a_piece_first_appears(emu, oracle, nt, lds):
    """L = 1: no pair; 2: the first pairs across the nick; 4, 5: around the first hairpin inside a strand (TURN = 3);
    12 .. 14: the first multiloop whose helix encloses the nick; 17 and 25: one odd, one even.  GC-rich letters so that the
    helices these shapes need do form.  (The workspace kernel with 128 threads: test_both_kernels_bit_identical)"""
    rng = np.random.default_rng(100 + nt + lds)
    for L in (1, 2, 4, 5, 12, 13, 14, 17, 25):
        _check(emu, oracle, [_rand(rng, L, "GCGCAU")], nt, lds)


def test_lds_bound_and_the_first_length_beyond_it(emu, oracle):
    """(the emulation's cost is its barriers, which grow with the workgroup: the longest cases run with 64 threads only)"""
    rng = np.random.default_rng(7)
    M = emu.lds_max
    assert M >= 36                                     # the reference's standard example fits the LDS path
    _check(emu, oracle, [_rand(rng, M)], 64, lds=True)
    _check(emu, oracle, [_rand(rng, M + 1)], 64, lds=False)


def test_a_longer_sequence_leaves_the_lds_kernel_at_once(emu):
    F4, st = emu.fold(["A" * (emu.lds_max + 1)], nt=64, lds=True)
    assert list(st) == [2] and not F4.any()            # ST_TRACEBACK: the host never launches it


def test_both_kernels_bit_identical(emu, oracle):
    rng = np.random.default_rng(8)
    seqs = [_rand(rng, 25), _rand(rng, 25, "GC"), "GGGAUCCCAGGGAUCCCAGGGAUCC"]
    a = _check(emu, oracle, seqs, 128, lds=True)
    b = _check(emu, oracle, seqs, 128, lds=False)
    c, _ = emu.fold(seqs, nt=64, lds=False)
    assert a.tobytes() == b.tobytes() == c.tobytes()


@pytest.mark.parametrize("L,nt", [(2, 64), (5, 64), (13, 64), (14, 64), (25, 64), (32, 64), (14, 128)])
def test_bit_identical_to_the_pair_kernel(emu, pair_emu, L, nt):
    """one body, two layouts: both self-dimer kernels return the bytes of cofold_pf_lds_kernel on s & s, all four columns
    (32 is the longest s whose doubled pair that kernel takes)"""
    pair = pair_emu
    assert 2 * L <= pair.max_len
    s = _rand(np.random.default_rng(300 + L + nt), L, "GCGCAU")
    want = pair.cofold([s + "&" + s], nt=nt)[2]
    for lds in (True, False):
        F4, st = emu.fold([s], nt=nt, lds=lds)
        assert not st.any()
        assert F4.tobytes() == want.tobytes(), (s, lds, F4, want)


def test_special_sequences(emu, oracle):
    rng = np.random.default_rng(9)
    F4 = _check(emu, oracle, ["A" * 9], 64)            # cannot pair at all
    assert F4[0, 2] == 999.0
    _check(emu, oracle, [_rand(rng, 14, "GC")], 128)
    # self-complementary: the duplex takes most strands (the values themselves are checked against the oracle in _check; the
    # longer palindromes also fold into a hairpin of their own, which keeps a few percent as monomers), the log term stays finite
    for pal in ("GGGAUCCC", "GGGGAUAUCCCC", "GCGCGCGCAUAUGCGCGCGC"):
        F4 = _check(emu, oracle, [pal], 64)
        f = _frac(F4[0])
        bonus = float(es.kTlog_monomer_fraction(f))
        print(pal, "oligo_fraction", f, "bonus", bonus)
        assert 0.9 < f < 1.0 and np.isfinite(bonus) and bonus > 0


def test_bad_letter_sets_that_row_only(emu, oracle):
    seqs = ["GGGAAACCGGUU", "GGGANACCGGUU", "GCGAAACCGCUU"]
    for lds in (True, False):
        F4, st = emu.fold(seqs, nt=64, lds=lds)
        assert list(st) == [0, ST_BAD_CHAR, 0]
        assert not F4[1].any()
        for k in (0, 2):
            assert max(abs(g - o) for g, o in zip(F4[k], oracle.cofold_pf(seqs[k] + "&" + seqs[k]))) < F4_TOL
