"""Stochastic traceback (desirna_amd/csrc/fold_sample.hpp: pf_kernel + sample_kernel) in the CPU emulation, against the oracle:
exact structure probabilities by enumeration (tests/sampling_ref.py), pair frequencies against the forbidden-pair reference
(tests/pair_prob_ref.py), energies against oracle.eval_structure, and the contract of the random numbers (a sample depends on the
sequence, its seed and its index alone).  Seeds are fixed, so every outcome is fixed."""
import numpy as np
import pytest

from tests import pair_prob_ref as ppr
from tests import sampling_ref as sr
from tests.emu import emu_sampling as es

ST_OK, ST_BAD_CHAR = 0, 1
SHORT = ["GGGAAACGGAAACCGA", "GGACGAAAGCAAAACC", "GCAAGCAAAGCAAAGC", "GGGGAAAACCCC", "GCGCAAAAGCGCAAAAGCGC"]
# structures with a multiloop hold 62.3 % of this one's mass (1131 structures; enumeration on the CPU, has_multiloop)
MULTILOOP = "GGGCGAAAGCGCGAAAGCCC"
S_EXACT, S_LONG = 20000, 1024


@pytest.fixture(scope="module")
def emu(blob):
    return es.EmuSampling(blob)


# ---------------------------------------------------------------- smallest shapes

@pytest.fixture(scope="module")
def tiny():
    return es.sample_many([(["A"], 256, 3), (["ACGU"], 256, 4), (["GAAAC"], 20000, 5)], G=4)


def test_one_nucleotide(tiny):
    assert set(es.strings(tiny[0]["ss"])[0]) == {"."} and tiny[0]["status"][0] == ST_OK
    assert (tiny[0]["E"] == 0).all()


def test_four_nucleotides(tiny):
    assert set(es.strings(tiny[1]["ss"])[0]) == {"...."} and (tiny[1]["E"] == 0).all()


def test_smallest_hairpin(tiny, oracle):
    ss = es.strings(tiny[2]["ss"])[0]
    dist = sr.exact_distribution(oracle, "GAAAC")
    assert set(dist) == {".....", "(...)"} and set(ss) <= set(dist)
    assert sr.meets(ss.count("(...)") / len(ss), dist["(...)"], len(ss))
    assert not sr.check_distribution(ss, dist, p_min=0.0)


# ---------------------------------------------------------------- exact distributions

@pytest.fixture(scope="module")
def exact():
    seqs = SHORT + [MULTILOOP]
    res = es.sample_many([([s], S_EXACT, 100 + k) for k, s in enumerate(seqs)], G=8)
    return {s: r for s, r in zip(seqs, res)}


@pytest.mark.parametrize("seq", SHORT + [MULTILOOP])
def test_exact_distribution(exact, oracle, seq):
    """every structure with p >= 1e-3 and the bucket of all others meet |f - p| <= 6 sqrt(max(p (1 - p), 10 / S) / S); every sampled
    string is a member of the enumeration"""
    r = exact[seq]
    assert r["status"][0] == ST_OK
    ss = es.strings(r["ss"])[0]
    assert len(ss) == S_EXACT
    dist = sr.exact_distribution(oracle, seq)
    assert abs(sum(dist.values()) - 1.0) < 1e-9          # the walk and the oracle's fill agree on Z
    bad = sr.check_distribution(ss, dist)
    assert not bad, bad
    for s in set(ss):
        k = ss.index(s)
        assert r["E"][0, k] == oracle.eval_structure(seq, s)


def test_multiloop_share(oracle):
    dist = sr.exact_distribution(oracle, MULTILOOP)
    share = sum(p for s, p in dist.items() if sr.has_multiloop(s))
    assert len(MULTILOOP) <= 26 and share >= 0.01
    assert abs(share - 0.6233) < 1e-3


# ---------------------------------------------------------------- longer sequences

def long_cases(eterna_solutions):
    """golden Eterna solutions of 70-80 and about 130 nt (candidate lists beyond one and beyond two chunks of 64), and a random 130-mer"""
    by_len = {}
    for r in eterna_solutions:
        by_len.setdefault(len(r["sequence"]), r["sequence"])
    return [by_len[75], by_len[123], ppr.rand_seq(np.random.default_rng(130), 130)]


@pytest.fixture(scope="module")
def longer(eterna_solutions):
    seqs = long_cases(eterna_solutions)
    res = es.sample_many([([s], S_LONG, 200 + k) for k, s in enumerate(seqs)], G=8)
    return list(zip(seqs, res))


@pytest.mark.parametrize("k", range(3))
def test_longer_sequences(longer, oracle, k):
    seq, r = longer[k]
    assert r["status"][0] == ST_OK
    ss = es.strings(r["ss"])[0]
    assert len(ss) == S_LONG and all(sr.well_formed(seq, s) for s in ss)
    for s in set(ss):
        assert r["E"][0, ss.index(s)] == oracle.eval_structure(seq, s)
    pairs = ppr.allowed_pairs(seq)
    P = ppr.reference_matrix(oracle, seq, pairs)
    bad = sr.check_pair_frequencies(ss, P, pairs)
    assert not bad, bad
    assert abs(r["Epf"][0] - oracle.pf(seq)) < 1e-6


# ---------------------------------------------------------------- contract

A16, B16, C16 = SHORT[0], SHORT[1], SHORT[2]


@pytest.fixture(scope="module")
def contract(eterna_solutions):
    s75 = long_cases(eterna_solutions)[0]
    jobs = {
        "nt64": ([A16, B16], 48, 7, 64, 1, None),
        "nt128": ([A16, B16], 48, 7, 128, 1, None),
        "nt64_75": ([s75], 24, 9, 64, 1, None),
        "nt128_75": ([s75], 24, 9, 128, 3, None),
        "prefix": ([A16, B16], 16, 7, 64, 1, None),
        "moved": ([C16, B16, A16], 48, np.array([99, 8, 7], dtype=np.uint64), 64, 2, None),
        "seed": ([A16], 48, 8, 64, 1, None),
        "bad": ([A16, "GGACGAAXGCAAAACC", B16], 48, np.array([7, 1, 8], dtype=np.uint64), 64, 1, None),
    }
    res = es.run_jobs(list(jobs.values()))
    return dict(zip(jobs, res))


def test_same_bytes_64_and_128_threads(contract):
    for a, b in (("nt64", "nt128"), ("nt64_75", "nt128_75")):
        assert contract[a]["ss"].all()                    # every sample written
        assert (contract[a]["ss"] == contract[b]["ss"]).all() and (contract[a]["E"] == contract[b]["E"]).all()


def test_first_samples_of_a_longer_call(contract):
    assert (contract["nt64"]["ss"][:, :16] == contract["prefix"]["ss"]).all()
    assert (contract["nt64"]["E"][:, :16] == contract["prefix"]["E"]).all()


def test_neighbours_and_position_do_not_matter(contract):
    base, moved = contract["nt64"], contract["moved"]
    assert (moved["ss"][2] == base["ss"][0]).all() and (moved["ss"][1] == base["ss"][1]).all()
    assert (moved["E"][2] == base["E"][0]).all() and (moved["E"][1] == base["E"][1]).all()


def test_two_seeds_differ(contract):
    assert (contract["seed"]["ss"][0] != contract["nt64"]["ss"][0]).any()


def test_bad_letter_leaves_the_neighbours(contract):
    bad, base = contract["bad"], contract["nt64"]
    assert list(bad["status"]) == [ST_OK, ST_BAD_CHAR, ST_OK]
    assert not bad["ss"][1].any() and (bad["E"][1] == -7).all()          # nothing written
    assert (bad["ss"][0] == base["ss"][0]).all() and (bad["ss"][2] == base["ss"][1]).all()


def test_random_numbers(emu):
    """u(seed, s, k): 53 bits in [0, 1), a function of its three arguments (written down in DESIGN 3.12)"""
    M, G = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def u(seed, s, k):
        return (mix((mix((mix((seed + G) & M) + (s + 1) * G) & M) + (k + 1) * G) & M) >> 11) * 2.0 ** -53

    for seed, s, k in [(0, 0, 0), (1, 2, 3), (2 ** 64 - 1, 19999, 700), (12345678901234567, 5, 0)]:
        v = emu.u(seed, s, k)
        assert v == u(seed, s, k) and 0.0 <= v < 1.0
    vals = np.array([emu.u(11, s, k) for s in range(64) for k in range(64)])
    assert len(set(vals)) == vals.size and abs(vals.mean() - 0.5) < 6 * np.sqrt(1 / 12 / vals.size)
