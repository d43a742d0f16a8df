"""The tails of the fused launch (score_fused_kernel): the MFE traceback -- shape table by one packed load per scan round, model
constants read once, the interior scan by groups of rounds, the sector queue on LDS atomics -- and the partition function's main
and helper roles beside it (Epf bitwise equal however the fold is run).  Everything goes through score_batch_device and asserts
the fused launch (last_fused).

Constructed records (tests/constructs.py) put a hit into every scan round, every table-driven kind and every hairpin table:
thinned_interior(), small(), hairpin() -- which holds a record for every entry of special_hairpins() -- and multiloop(), padded to
125 nt (the shortest the fused launch takes) and 200 nt (the longest) with the three OFFSET_RULES.  Emfe, structure and E(target)
are bit-exact against the oracle, Epf within 1e-9 kcal/mol (summation order only)."""
import ctypes as C_

import numpy as np
import pytest

from tests import constructs as C

pytestmark = pytest.mark.gpu

EPF_TOL = 1e-9
PER_CALL = 32


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=64, max_L=200, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def records():
    return C.thinned_interior() + C.small() + C.hairpin() + C.multiloop()


class _Hip:
    """the four HIP runtime calls the device entry point needs around it, taken from the runtime the engine's library is linked
    to (a second runtime in the process, such as a tensor library's own copy, would not see the engine's context)"""

    def __init__(self, lib):
        self.L = lib
        lib.hipMalloc.argtypes, lib.hipMalloc.restype = [C_.POINTER(C_.c_void_p), C_.c_size_t], C_.c_int
        lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [C_.c_void_p, C_.c_void_p, C_.c_size_t, C_.c_int], C_.c_int
        lib.hipFree.argtypes, lib.hipFree.restype = [C_.c_void_p], C_.c_int
        lib.hipDeviceSynchronize.argtypes, lib.hipDeviceSynchronize.restype = [], C_.c_int

    def upload(self, a):
        p = C_.c_void_p()
        assert self.L.hipMalloc(C_.byref(p), a.nbytes) == 0
        assert self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0          # host to device
        return p

    def download(self, p, a):
        assert self.L.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0          # device to host
        return a


def _score(eng, seqs, targets, pk=False):
    """seqs through score_batch_device (device buffers made and freed here): Epf, Emfe, structures, Ed[R, len(targets)]"""
    from desirna_amd import engine as E
    R, L = len(seqs), len(seqs[0])
    hip = _Hip(eng._L)
    eng.set_targets(targets)
    host = [np.frombuffer("".join(seqs).encode(), dtype=np.uint8).copy(), np.zeros(R), np.zeros(R, dtype=np.int32),
            np.zeros((R, L), dtype=np.uint8), np.zeros((R, len(targets)), dtype=np.int32)]
    dev = [hip.upload(a) for a in host]
    try:
        assert hip.L.hipDeviceSynchronize() == 0
        flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL | (E.NEED_PK if pk else 0)
        eng.score_batch_device(dev[0], R, L, flags, dev[1], dev[2], dev[3], dev[4])
        assert hip.L.hipDeviceSynchronize() == 0
        Epf, Emfe, ss, Ed = (hip.download(p, a) for p, a in zip(dev[1:], host[1:]))
    finally:
        for p in dev:
            hip.L.hipFree(p)
    return Epf, Emfe, [bytes(r).decode("ascii") for r in ss], Ed


def _rand(rng, L):
    return "".join(rng.choice(list("ACGU"), L))


def _same(a, b):
    return (a[0].view(np.int64) == b[0].view(np.int64)).all() and (a[1] == b[1]).all() and a[2] == b[2] and (a[3] == b[3]).all()


@pytest.mark.parametrize("k", C.OFFSET_RULES)
@pytest.mark.parametrize("L", [125, 200])
def test_constructs_fused(eng, oracle, records, L, k):
    frames = [C.pad(r, L, k) for r in records]
    assert len(frames) == len(records) > 6000                # every record fits the shorter frame
    worst = 0.0
    for b in range(0, len(frames), PER_CALL):
        sub = frames[b:b + PER_CALL]
        seqs, tgts = [f[0] for f in sub], [f[1] for f in sub]
        Epf, Emfe, ss, Ed = oracle.score_batch(seqs, tgts)
        got = _score(eng, seqs, tgts)
        assert eng.get_option("last_fused") == 1 and eng.get_option("last_workgroups") == 4 * len(sub)
        for q in range(len(sub)):
            name = records[b + q].name
            assert got[2][q] == ss[q], (name, sub[q][2], got[2][q], ss[q])
            assert int(got[1][q]) == int(Emfe[q]), (name, sub[q][2])
        assert (got[3] == Ed).all(), records[b + int(np.argwhere(got[3] != Ed)[0][0])].name
        d = np.abs(got[0] - Epf)
        worst = max(worst, float(d.max()))
        assert d.max() < EPF_TOL, (records[b + int(d.argmax())].name, float(d.max()))
    assert eng.get_option("sync_fallbacks") == 0
    print("L %d offset rule %d: %d records, max |Epf - oracle| %.3g" % (L, k, len(frames), worst))


@pytest.mark.parametrize("R", [1, 8, 9])                      # 9: the grid is rounded up to a multiple of 8 blocks per role
@pytest.mark.parametrize("L", [125, 126, 199, 200])
def test_random_batches_and_paths(eng, oracle, L, R):
    rng = np.random.default_rng(1000 * L + R)
    seqs = [_rand(rng, L) for _ in range(R)]
    tgts = [oracle.mfe(seqs[0])[0]]
    Epf, Emfe, ss, Ed = oracle.score_batch(seqs, tgts)
    a = _score(eng, seqs, tgts)
    assert eng.get_option("last_fused") == 1 and eng.get_option("last_workgroups") == 4 * R
    assert a[2] == list(ss) and (a[1] == Emfe).all() and (a[3] == Ed).all()
    assert np.abs(a[0] - Epf).max() < EPF_TOL
    # Epf does not depend on how the fold was run: two launches, then no helper workgroup
    try:
        eng.set_option("fused", 0)
        b = _score(eng, seqs, tgts)
        assert eng.get_option("last_fused") == 0 and eng.get_option("last_workgroups") == 4 * R
        eng.set_option("pf_helper", 0)
        c = _score(eng, seqs, tgts)
        assert eng.get_option("last_fused") == 0 and eng.get_option("last_workgroups") == 3 * R
    finally:
        eng.set_option("fused", 1)
        eng.set_option("pf_helper", 1)
    assert _same(a, b) and _same(a, c)
    assert eng.get_option("sync_fallbacks") == 0


def test_stale_workspace(eng, oracle):
    """two calls on one engine with different sequences: the second finds the first one's tables (and hand-over lines) in its
    workspace and must answer as a fresh engine does"""
    from desirna_amd import engine
    rng = np.random.default_rng(77)
    L, R = 200, 9
    first, second = [_rand(rng, L) for _ in range(R)], [_rand(rng, L) for _ in range(R)]
    tgts = [oracle.mfe(second[0])[0]]
    _score(eng, first, tgts)
    a = _score(eng, second, tgts)
    assert eng.get_option("last_fused") == 1
    fresh = engine.Engine(max_R=64, max_L=200, device=0)
    try:
        b = _score(fresh, second, tgts)
        assert fresh.get_option("last_fused") == 1
    finally:
        fresh.close()
    assert _same(a, b)
    Epf, Emfe, ss, Ed = oracle.score_batch(second, tgts)
    assert a[2] == list(ss) and (a[1] == Emfe).all() and (a[3] == Ed).all() and np.abs(a[0] - Epf).max() < EPF_TOL


def test_pseudoknot_rounds_170(eng, oracle):
    """the re-folds of the pseudoknot heuristic (masked positions in fill and traceback) at the shortest length at which they
    take the fused launch"""
    rng = np.random.default_rng(170)
    L, R = 170, 8
    seqs = [_rand(rng, L) for _ in range(R)]
    tgts = [oracle.mfe(seqs[0])[0]]
    Epf, Emfe, ss, Ed = oracle.score_batch(seqs, tgts)
    a = _score(eng, seqs, tgts, pk=True)
    assert eng.get_option("last_fused") == 1
    want = [oracle.pk_struct(s, x) for s, x in zip(seqs, ss)]
    assert a[2] == want and (a[1] == Emfe).all() and (a[3] == Ed).all() and np.abs(a[0] - Epf).max() < EPF_TOL
    assert any("[" in w for w in want)                       # at least one sequence goes into a second round's traceback
