"""The reference of the accessible-region tests held to the pinned fill (CPU, oracle only): F[not i] by ENUMERATION
(tests/access_ref.py: every structure of the fill's set weighed by oracle.boltzmann_weight, the ones that pair i left out)
against oracle.pf_forbid(seq, i, 0) at every position, on the twelve sparse 100 - 260 nt cases and twelve dense 9 - 16 nt
ones.  Reference against reference: 1e-11 kcal/mol.  The case conditions (at most 2e5 structures, the count equal to
oracle.count_structures, a tested mask that opens more than 0.1 kcal/mol) are checked on the reference alone; a case that misses
one is an error in the case list."""
import numpy as np
import pytest

from tests import access_ref as ar

REF_TOL = 1e-11


def _cases():
    return list(ar.sparse_cases().items()) + [("dense_%d_%s" % (len(s), s), s) for s in ar.dense_reference_cases()]


def test_case_lists():
    sparse, dense = ar.sparse_cases(), ar.dense_reference_cases()
    assert len(sparse) == 12 and all(100 <= len(s) <= 260 for s in sparse.values())
    assert len(dense) == 12 == len(set(dense)) and all(9 <= len(s) <= 16 for s in dense)
    kernel = ar.dense_kernel_cases()
    assert len(kernel) == 6 and set(ar.TIGHT) <= set(kernel) and all(9 <= len(s) <= 16 for s in kernel)


@pytest.mark.parametrize("name,seq", _cases(), ids=[c[0] for c in _cases()])
def test_enumeration_equals_the_masked_fill(oracle, name, seq):
    n = len(seq)
    ens = ar.Ensemble(oracle, seq)                         # raises above the cap or on unequal counts
    assert ens.count == oracle.count_structures(seq) <= ar.CAP
    F = ar.check_case(ens, ar.single_masks(n))             # raises unless a position costs more than 0.1 kcal/mol to free
    ref = oracle.pf_forbid(seq, list(range(1, n + 1)), 0)
    assert abs(ens.F0 - oracle.pf(seq)) <= REF_TOL
    assert abs(ens.F0 - oracle.pf_forbid(seq, 0, 0)) <= REF_TOL
    assert np.abs(F - ref).max() <= REF_TOL
    assert (F >= ens.F0 - 1e-12).all()                     # freeing a position never lowers the free energy


def test_masks_compose(oracle):
    """what the enumeration adds to pf_forbid: several positions at once.  A mask over positions that pair with nothing changes
    nothing, all ones leaves the open chain (F = 0), and a larger mask never costs less"""
    seq = ar.sparse_cases()["seeded_100_12"]
    ens = ar.Ensemble(oracle, seq)
    n = len(seq)
    lone = np.array([[c == "A" for c in seq]], dtype=np.uint8)             # no U anywhere: A pairs with nothing
    assert ens.free_energy(lone)[0] == ens.F0
    assert abs(ens.free_energy(np.ones((1, n), dtype=np.uint8))[0]) < 1e-12
    w8, w4 = ar.window_masks(n, 8), ar.window_masks(n, 4)
    F8, F4 = ens.free_energy(w8), ens.free_energy(w4)
    for a in range(w8.shape[0]):
        assert F4[a] <= F8[a] + 1e-12 and F4[a + 4] <= F8[a] + 1e-12
    assert (F8 - ens.F0 > ar.MIN_EOPEN).sum() >= 20
