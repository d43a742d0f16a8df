"""Two-strand stochastic traceback (desirna_amd/csrc/fold_cofold_sample.hpp: cofold_pf_kernel + cofold_columns_kernel +
cofold_sample_kernel) in the CPU emulation, against the oracle: exact structure probabilities by enumeration of every co-fold
structure (tests/cofold_sampling_ref.py), connected fractions against the oracle's FcAB - FAB, pair frequencies against the
forbidden-pair reference (tests/pair_prob_ref.py), energies against oracle.eval_structure with the nick, and the contract of the
random numbers (a sample depends on the two sequences, the pair's seed and its index alone).  Seeds are fixed, so every outcome
is fixed."""
import numpy as np
import pytest

from tests import cofold_sampling_ref as cr
from tests import pair_prob_ref as ppr
from tests import sampling_ref as sr
from tests.emu import emu_cofold_sampling as ec

ST_OK, ST_BAD_CHAR = 0, 1
NAMED = [c for c, _ in cr.NAMED]
HOMODIMERS = [c for c in NAMED if c.split("&")[0] == c.split("&")[1]]
S_EXACT, S_LONG = 20000, 1024
# (strand lengths, seed of pair_prob_ref.two_strand_case(planted=True), seed of pair_prob_ref.sampled_pairs): seeds for which the
# sampled set is informative on the reference alone (asserted below)
LONG = [((18, 18), 300, 0), ((25, 11), 300, 0), ((50, 50), 300, 0)]


def long_case(shape, seed):
    return ppr.two_strand_case(np.random.default_rng(seed), shape[0], shape[1], "ACGU", True)


def samples_of(r, k=0):
    return ec.strings(r["ss"], r["cut"])[k]


def check_energies(oracle, pair, r, k=0):
    flat, cut = ppr.split(pair)
    ss = samples_of(r, k)
    for s in set(ss):
        assert r["E"][k, ss.index(s)] == oracle.eval_structure(flat, s.replace("&", ""), cut), (pair, s)


# ---------------------------------------------------------------- smallest shapes

TINY = ["A&A", "A&U", "G&C", "GAAAC&A", "CUCC&CUCC"]


@pytest.fixture(scope="module")
def tiny():
    res = ec.sample_many([([p], S_EXACT if p in ("A&U", "G&C", "GAAAC&A") else 256, 3 + k) for k, p in enumerate(TINY)], G=4)
    return dict(zip(TINY, res))


def test_two_nucleotides_that_cannot_pair(tiny):
    r = tiny["A&A"]
    assert r["status"][0] == ST_OK and set(samples_of(r)) == {".&."} and (r["E"] == 0).all()


@pytest.mark.parametrize("pair", ["A&U", "G&C"])
def test_one_joining_pair_that_encloses_nothing(tiny, oracle, pair):
    r = tiny[pair]
    dist, F = cr.exact_distribution(oracle, pair)
    assert set(dist) == {".&.", "(&)"} and cr.enters(oracle, pair, F)
    ss = samples_of(r)
    assert len(ss) == S_EXACT and not sr.check_distribution(ss, dist, p_min=0.0)
    assert sr.meets(ss.count("(&)") / len(ss), cr.connected_fraction(oracle, pair), len(ss))
    check_energies(oracle, pair, r)


def test_hairpin_beside_an_unfoldable_strand(tiny, oracle):
    r = tiny["GAAAC&A"]
    dist, F = cr.exact_distribution(oracle, "GAAAC&A")
    assert set(dist) == {".....&.", "(...)&."} and cr.enters(oracle, "GAAAC&A", F)
    ss = samples_of(r)
    assert not sr.check_distribution(ss, dist, p_min=0.0)
    assert sr.meets(ss.count("(...)&.") / len(ss), dist["(...)&."], len(ss))
    check_energies(oracle, "GAAAC&A", r)


def test_one_structure(tiny, oracle):
    r = tiny["CUCC&CUCC"]
    assert set(cr.exact_distribution(oracle, "CUCC&CUCC")[0]) == {"....&...."}
    assert set(samples_of(r)) == {"....&...."} and (r["E"] == 0).all()


# ---------------------------------------------------------------- exact distributions

@pytest.fixture(scope="module")
def exact():
    res = ec.sample_many([([p], S_EXACT, 100 + k) for k, p in enumerate(NAMED)], G=8)
    return dict(zip(NAMED, res))


@pytest.fixture(scope="module")
def dists(oracle):
    return {p: cr.exact_distribution(oracle, p) for p in NAMED}


@pytest.mark.parametrize("pair,count", cr.NAMED)
def test_exact_distribution(exact, dists, oracle, pair, count):
    """every named case enters (|F_enum - FAB| < 1e-6 kcal/mol); every sampled string is a member of the enumeration; every structure
    with p >= 1e-3 and the bucket of all others meet |f - p| <= 6 sqrt(max(p (1 - p), 10 / S) / S); so does the connected fraction
    against exp(-(FcAB - FAB) / kT); the energy of every distinct sample is the oracle's"""
    r = exact[pair]
    dist, F = dists[pair]
    assert len(dist) == count and abs(sum(dist.values()) - 1.0) < 1e-9
    assert cr.enters(oracle, pair, F), (pair, F, oracle.cofold_pf(pair)[3])
    assert r["status"][0] == ST_OK
    assert np.abs(r["F4"][0] - np.array(oracle.cofold_pf(pair))).max() < 1e-6
    ss = samples_of(r)
    assert len(ss) == S_EXACT
    bad = sr.check_distribution(ss, dist)
    assert not bad, bad
    f_conn, p_conn = sum(cr.is_connected(s) for s in ss) / S_EXACT, cr.connected_fraction(oracle, pair)
    print(pair, "connected f = %.5f p = %.5f" % (f_conn, p_conn))
    assert sr.meets(f_conn, p_conn, S_EXACT), (f_conn, p_conn)
    check_energies(oracle, pair, r)


@pytest.mark.parametrize("pair", HOMODIMERS)
def test_homodimer_rotation(exact, dists, pair):
    """X&X: a structure and its rotation are two structures of equal probability -- the distribution the samples are held to has
    that symmetry, and both members of every heavy couple are drawn at its rate"""
    dist = dists[pair][0]
    assert all(cr.rotated(s) in dist and abs(dist[cr.rotated(s)] - p) < 1e-12 for s, p in dist.items())
    ss = samples_of(exact[pair])
    assert not sr.check_distribution(ss, dist)
    couples = [s for s, p in dist.items() if p >= 1e-3 and cr.rotated(s) != s]
    assert couples
    for s in couples:
        assert sr.meets(ss.count(s) / len(ss), dist[s], len(ss)) and sr.meets(ss.count(cr.rotated(s)) / len(ss), dist[s], len(ss))


def test_multiloop_share(dists):
    """the 14+11 case keeps covering the multiloop candidates of a joining pair, from the enumeration alone"""
    share = cr.nick_multiloop_share(dists[cr.MULTILOOP][0])
    print("multiloop share %.4f" % share)
    assert share >= 0.1


# ---------------------------------------------------------------- strands that cannot pair with each other

CANNOT = "GGGAAACGGAAACCGA&AAAAAA"


@pytest.fixture(scope="module")
def cannot():
    return ec.sample_many([([CANNOT], S_EXACT, 77)], G=8)[0]


def test_strands_that_cannot_pair(cannot, oracle):
    """nothing joins {G, C} to A: no sample is connected, and strand A's part of the strings follows the one-strand distribution"""
    ss = samples_of(cannot)
    a = CANNOT.split("&")[0]
    assert len(ss) == S_EXACT and not any(cr.is_connected(s) for s in ss)
    assert all(s.split("&")[1] == "." * 6 for s in ss)
    bad = sr.check_distribution([s.split("&")[0] for s in ss], sr.exact_distribution(oracle, a))
    assert not bad, bad
    check_energies(oracle, CANNOT, cannot)


# ---------------------------------------------------------------- longer pairs

@pytest.fixture(scope="module")
def longer():
    pairs = [long_case(shape, cs) for shape, cs, _ in LONG]
    res = ec.sample_many([([p], S_LONG, 200 + k) for k, p in enumerate(pairs)], G=8)
    return list(zip(pairs, res))


@pytest.mark.parametrize("k", range(len(LONG)))
def test_longer_pairs(longer, oracle, k):
    pair, r = longer[k]
    assert r["status"][0] == ST_OK
    ss = samples_of(r)
    assert len(ss) == S_LONG and all(cr.well_formed(pair, s) for s in ss)
    check_energies(oracle, pair, r)
    pairs = ppr.sampled_pairs(oracle, pair, LONG[k][2])
    P = ppr.reference_matrix(oracle, pair, pairs)
    assert ppr.sample_is_informative(pair, pairs, [P[i, j] for i, j in pairs]), pair
    bad = sr.check_pair_frequencies([s.replace("&", "") for s in ss], P, pairs)
    assert not bad, bad
    assert np.abs(r["F4"][0] - np.array(oracle.cofold_pf(pair))).max() < 1e-6


# ---------------------------------------------------------------- contract

@pytest.fixture(scope="module")
def contract():
    a18, b18, c18 = (long_case((18, 18), s) for s in (300, 301, 302))
    p50 = long_case((50, 50), 300)
    bad = b18[:5] + "X" + b18[6:]
    jobs = {
        "nt64": ([a18, b18], 48, 7, 64, 1, None),
        "nt128": ([a18, b18], 48, 7, 128, 1, None),
        "g2": ([a18, b18], 48, 7, 64, 2, None),
        "g3": ([a18, b18], 48, 7, 128, 3, None),
        "nt64_50": ([p50], 24, 9, 64, 1, None),
        "nt128_50": ([p50], 24, 9, 128, 3, None),
        "prefix": ([a18, b18], 16, 7, 64, 1, None),
        "moved": ([c18, b18, a18], 48, np.array([99, 8, 7], dtype=np.uint64), 64, 2, None),
        "zeros": ([a18, b18], 48, 7, 64, 1, None, 0x00),
        "seed": ([a18], 48, 8, 64, 1, None),
        "bad": ([a18, bad, b18], 48, np.array([7, 1, 8], dtype=np.uint64), 64, 1, None),
    }
    res = ec.run_jobs(list(jobs.values()))
    return dict(zip(jobs, res))


def same(a, b):
    return (a["ss"] == b["ss"]).all() and (a["E"] == b["E"]).all()


def test_same_bytes_64_and_128_threads_and_any_grid(contract):
    assert contract["nt64"]["ss"].all() and contract["nt64_50"]["ss"].all()          # every sample written
    for other in ("nt128", "g2", "g3"):
        assert same(contract["nt64"], contract[other]), other
    assert same(contract["nt64_50"], contract["nt128_50"])


def test_first_samples_of_a_longer_call(contract):
    assert (contract["nt64"]["ss"][:, :16] == contract["prefix"]["ss"]).all()
    assert (contract["nt64"]["E"][:, :16] == contract["prefix"]["E"]).all()


def test_neighbours_and_position_do_not_matter(contract):
    base, moved = contract["nt64"], contract["moved"]
    assert (moved["ss"][2] == base["ss"][0]).all() and (moved["ss"][1] == base["ss"][1]).all()
    assert (moved["E"][2] == base["E"][0]).all() and (moved["E"][1] == base["E"][1]).all()


def test_what_the_slot_held_does_not_matter(contract):
    """the other tests start slot and columns as NaN; here they start as zeros"""
    assert same(contract["nt64"], contract["zeros"])


def test_two_seeds_differ(contract):
    assert (contract["seed"]["ss"][0] != contract["nt64"]["ss"][0]).any()


def test_bad_letter_leaves_the_neighbours(contract):
    bad, base = contract["bad"], contract["nt64"]
    assert list(bad["status"]) == [ST_OK, ST_BAD_CHAR, ST_OK]
    assert not bad["ss"][1].any() and (bad["E"][1] == -7).all()          # nothing written
    assert (bad["ss"][0] == base["ss"][0]).all() and (bad["ss"][2] == base["ss"][1]).all()
