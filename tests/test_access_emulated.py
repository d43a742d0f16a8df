"""The two kernels of the partition function with positions held unpaired in the CPU emulation (tests/emu/emu_access.cpp:
pf_kernel<NT, true> at 64, 128 and 256 threads -- path a -- and access_lds_kernel at 64 and 128 -- path b --, unmodified), against
enumeration (tests/access_ref.py) and the pinned masked fill oracle.pf_forbid.  1e-9 kcal/mol against a reference, bit equality
where the same code sums in the same order.

The dense cases aim at the one trap of the feature: a masked nucleotide is still that nucleotide next to a pair, so the mismatch,
dangle, special-hairpin and small-loop look-ups must keep reading the letters; read with the pairing code 4 they would index past
their tables.  The masks over exactly the unpaired neighbours of the MFE structure's pairs, on stems that sit directly against
their loops and ends, are where that shows.

Every emulated fold of the module runs once, spread over worker processes (one job per process at a time)."""
import numpy as np
import pytest

from tests import access_ref as ar, pair_prob_ref
from tests.emu import emu_access as ea

TOL = 1e-9                                            # EPF_TOL_ORACLE: an emulated F against the oracle or the enumeration
LDS_MAX = ea.lds_max()
CONFIGS = [(False, nt) for nt in ea.GENERAL_NT] + [(True, nt) for nt in ea.LDS_NT]
IDS = ["%s%d" % ("b" if lds else "a", nt) for lds, nt in CONFIGS]
NO_PAIR_5 = ["GGGAA", "ACGUA"]                        # five nucleotides whose ends cannot pair: the open chain alone
A_ALONE = (63, 64, 65, 129)
ST_OK, ST_TRACEBACK = 0, 2


def _rand(n, tag, alphabet="ACGU"):
    return pair_prob_ref.rand_seq(np.random.default_rng([ar.SEED, 3, tag, n]), n, alphabet)


def _position_masks(n):
    return ar.mask_rows(n, [[p] for p in ar.inner_positions(n, 0)])


SPARSE = {k: ar.sparse_cases()[k] for k in ("seeded_100_12", "seeded_130_13")}
CROSS = {n: _rand(n, 1) for n in (24, 36, 64)}        # path a against path b
NO_U = SPARSE["seeded_100_12"]                        # A, G and C only: an A pairs with nothing
ZERO_SEQS = ar.dense_kernel_cases() + [_rand(65, 0), NO_U]


def _nested_masks(n, seed):
    """ten pairs (mask, mask') with mask a subset of mask'"""
    small = ar.random_masks(n, 10, seed)
    return small, small | ar.random_masks(n, 10, seed + 1)


@pytest.fixture(scope="module")
def masks(oracle):
    m = {("dense", s): ar.dense_masks(oracle, s) for s in ar.dense_kernel_cases()}
    m.update({("five", s): np.concatenate([ar.single_masks(5), ar.random_masks(5, 4, 2), np.zeros((1, 5), np.uint8)]) for s in NO_PAIR_5})
    m.update({("pos", n): _position_masks(n) for n in A_ALONE + (LDS_MAX, LDS_MAX + 1)})
    m.update({("sparse", k): ar.window_masks(len(s), 8, every=4) for k, s in SPARSE.items()})
    m.update({("cross", n): ar.random_masks(n, 10, 5) for n in CROSS})
    n = len(NO_U)
    small, large = _nested_masks(n, 11)
    lone = np.array([[c == "A" for c in NO_U]], dtype=np.uint8)
    # rows: 0 all zero, 1 every A (cannot pair anyway), 2 all ones, then the ten nested pairs
    m["inv"] = np.concatenate([np.zeros((1, n), np.uint8), lone, np.ones((1, n), np.uint8), small, large])
    return m


@pytest.fixture(scope="module")
def folds(masks):
    """every emulated fold of the module: {key: (F (R, M), status (R, M))}"""
    jobs = {}
    for lds, nt in CONFIGS:
        for s in ar.dense_kernel_cases():
            jobs[("dense", s, lds, nt)] = ([s], masks[("dense", s)], nt, lds, True, None)
        for s in NO_PAIR_5:
            jobs[("five", s, lds, nt)] = ([s], masks[("five", s)], nt, lds, True, None)
        for n in (A_ALONE if not lds else (LDS_MAX, LDS_MAX + 1)):
            jobs[("pos", n, lds, nt)] = ([_rand(n, 0)], masks[("pos", n)], nt, lds, True, None)
        for k, s in SPARSE.items():
            if not lds or len(s) <= LDS_MAX:
                jobs[("sparse", k, lds, nt)] = ([s], masks[("sparse", k)], nt, lds, True, None)
        jobs[("inv", lds, nt)] = ([NO_U], masks["inv"], nt, lds, True, 7)          # (chunks of 7: launches that begin at slot 0 again)
    for nt in ea.GENERAL_NT:                          # the unmasked pf_kernel<NT>, and the masked instance under an all-zero mask
        jobs[("plain", nt)] = (ZERO_SEQS, None, nt, False, False, None)
        jobs[("zero", nt)] = (ZERO_SEQS, None, nt, False, True, None)
    for n, s in CROSS.items():
        for lds, nt in ((False, 128), (True, 128)):
            jobs[("cross", n, lds)] = ([s], masks[("cross", n)], nt, lds, True, None)
    keys = list(jobs)
    todo = []
    for k in keys:
        seqs, m, nt, lds, masked, chunk = jobs[k]
        if m is None:                                 # sequences of different lengths: one job each, an all-zero mask
            todo += [([s], np.zeros((1, len(s)), np.uint8), nt, lds, masked, chunk) for s in seqs]
        else:
            todo.append(jobs[k])
    res = iter(ea.run_jobs(todo))
    out = {}
    for k in keys:
        if jobs[k][1] is None:
            out[k] = [next(res) for _ in jobs[k][0]]
        else:
            out[k] = next(res)
    return out


@pytest.fixture(scope="module")
def ensembles(oracle):
    return {s: ar.Ensemble(oracle, s) for s in ar.dense_kernel_cases() + list(SPARSE.values())}


@pytest.mark.parametrize("lds,nt", CONFIGS, ids=IDS)
def test_five_nucleotides(folds, lds, nt):
    for s in NO_PAIR_5:
        F, st = folds[("five", s, lds, nt)]
        assert (st == ST_OK).all() and np.abs(F).max() < 1e-12


@pytest.mark.parametrize("lds,nt", CONFIGS, ids=IDS)
def test_dense_against_enumeration(folds, masks, ensembles, lds, nt):
    for s in ar.dense_kernel_cases():
        ref = ar.check_case(ensembles[s], masks[("dense", s)])          # the case's conditions, on the reference alone
        F, st = folds[("dense", s, lds, nt)]
        assert (st == ST_OK).all()
        assert np.abs(F[0] - ref).max() <= TOL, (s, np.abs(F[0] - ref).max())


@pytest.mark.parametrize("nt", ea.GENERAL_NT)
@pytest.mark.parametrize("n", A_ALONE)
def test_general_kernel_positions(folds, oracle, n, nt):
    seq = _rand(n, 0)
    ref = oracle.pf_forbid(seq, ar.inner_positions(n, 0), 0)
    assert (ref - oracle.pf(seq)).max() > ar.MIN_EOPEN
    F, st = folds[("pos", n, False, nt)]
    assert (st == ST_OK).all() and np.abs(F[0] - ref).max() <= TOL


@pytest.mark.parametrize("nt", ea.LDS_NT)
def test_lds_kernel_at_its_bound(folds, oracle, nt):
    seq = _rand(LDS_MAX, 0)
    ref = oracle.pf_forbid(seq, ar.inner_positions(LDS_MAX, 0), 0)
    assert (ref - oracle.pf(seq)).max() > ar.MIN_EOPEN
    F, st = folds[("pos", LDS_MAX, True, nt)]
    assert (st == ST_OK).all() and np.abs(F[0] - ref).max() <= TOL
    F, st = folds[("pos", LDS_MAX + 1, True, nt)]               # one nucleotide more: the kernel leaves at once
    assert (st == ST_TRACEBACK).all() and (F == 0.0).all()


@pytest.mark.parametrize("lds,nt", CONFIGS, ids=IDS)
def test_sparse_windows_against_enumeration(folds, masks, ensembles, lds, nt):
    ran = 0
    for k, s in SPARSE.items():
        if lds and len(s) > LDS_MAX:
            continue
        ref = ar.check_case(ensembles[s], masks[("sparse", k)])
        F, st = folds[("sparse", k, lds, nt)]
        assert (st == ST_OK).all() and np.abs(F[0] - ref).max() <= TOL, k
        ran += 1
    assert ran >= 1


@pytest.mark.parametrize("nt", ea.GENERAL_NT)
def test_zero_mask_is_the_unmasked_kernel(folds, nt):
    """path a: the masked instance under an all-zero mask sums what pf_kernel<NT> sums, in its order"""
    for seq, (F0, st0), (F, st) in zip(ZERO_SEQS, folds[("plain", nt)], folds[("zero", nt)]):
        assert st0[0, 0] == ST_OK and st[0, 0] == ST_OK
        assert F[0, 0] == F0[0, 0], seq


@pytest.mark.parametrize("nt", ea.LDS_NT)
def test_zero_mask_is_the_inside_half_of_the_edef_kernel(nt):
    """path b: the same body, layout and cut as edef_lds_kernel<NT, true>'s inside sweep -- the same bits (its F4[0])"""
    from tests.emu import emu_edef_lds
    seqs = ar.dense_kernel_cases()[:3] + [_rand(36, 2), _rand(64, 2)]
    ref = emu_edef_lds.edef_lds_many(seqs, ["." * len(s) for s in seqs], nt=nt)
    got = ea.run_jobs([([s], np.zeros((1, len(s)), np.uint8), nt, True, True, None) for s in seqs])
    for s, r, (F, st) in zip(seqs, ref, got):
        assert r[3] == ST_OK and st[0, 0] == ST_OK
        assert F[0, 0] == r[2][0], s


@pytest.mark.parametrize("lds,nt", CONFIGS, ids=IDS)
def test_invariants(folds, oracle, lds, nt):
    F, st = folds[("inv", lds, nt)]
    assert (st == ST_OK).all()
    F = F[0]
    assert abs(F[0] - oracle.pf(NO_U)) <= TOL
    assert F[1] == F[0]                                          # masking what cannot pair anyway: the same bits
    assert abs(F[2]) < 1e-12                                     # everything masked: the open chain
    small, large = F[3:13], F[13:23]
    assert (small <= large + 1e-12).all() and (F[0] <= small + 1e-12).all()
    assert (large - F[0]).max() > ar.MIN_EOPEN


def test_the_two_bodies_agree(folds, oracle):
    """dense random sequences of 24, 36 and 64 nt, ten random masks each: path a against path b, two independent bodies"""
    for n, s in CROSS.items():
        (Fa, sa), (Fb, sb) = folds[("cross", n, False)], folds[("cross", n, True)]
        assert (sa == ST_OK).all() and (sb == ST_OK).all()
        assert (Fa - oracle.pf(s)).max() > ar.MIN_EOPEN
        assert np.abs(Fa - Fb).max() <= TOL, n
