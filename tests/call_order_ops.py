"""The engine's public entry points as a table of operations on ONE engine size: what tests/test_call_order_gpu.py runs after
and before each other and on poisoned workspaces.  A plain helper module (no fixtures, no pytest configuration).

An operation (:class:`Op`) has a name, ``run(engine) -> tuple`` and ``anchor(oracle, result)``:

* ``run`` installs what the call needs (targets, ragged targets), makes one public ``Engine`` call on fixed seeded inputs, asserts
  the path the inputs' length was chosen for (where the engine exposes it) and returns everything the call returns except
  timings, as numpy arrays and strings.  Two results compare bit for bit (:func:`first_difference`).
* ``anchor`` compares the result with the oracle, within the bound the operation's own GPU test uses (named at each anchor), so
  that two equal wrong answers cannot pass.  ``reference(oracle)`` is the oracle's side alone; it also asserts that the inputs are
  not degenerate (a paired base in an MFE structure, a probability above 1e-3, a pair joining the strands), which
  tests/test_call_order_ops.py checks without a GPU.

``run`` is ``install`` + ``call(engine, seqs)``: the second half alone is the same call on other sequences (a failed call) or
without installing anything (do installed targets survive?).

Lengths sit on both sides of every path switch (the constants were read from the headers; ``path`` fails loudly if one moves):
fused launch 125 .. 200 nt (170 with the pseudoknot rounds), strips above 200, CO_LDS_MAX 64, SD_LDS_MAX 62, EDEF_LDS_HOST_MAX 40,
CO_EDEF_LDS_MAX 57, SUB_LDS_MAX 79, MEA_LDS_MAX 146, ACCESS_LDS_HOST_MAX 36."""
import ctypes as C_
import random

import numpy as np

from tests import pair_prob_ref as ppr

MAX_R, MAX_L = 16, 260
SEED = 20270
INF_E = 10000000                  # "no such structure" of the ranked folds
TARGET36 = "((((((.((((((((....))))).)).).))))))"
TARGET12 = "((((....))))"
CO_TARGET37 = "((((((((" + "." * 10 + "&" + "." * 10 + "))))))))"

EPF_TOL = 1e-9                    # tests/test_fused_tail_gpu.py, test_cofold_native_gpu.py (EPF_TOL_ORACLE), test_self_dimer_gpu.py (F4_TOL), test_access_gpu.py (TOL)
EDEF_TOL = 1e-10                  # tests/test_cofold_edef_emulated.py: defect and probabilities (test_edef_lds_gpu.py, test_pair_prob_reference_gpu.py, test_mea_gpu.py)
SAMPLE_EPF_TOL = 1e-6             # tests/test_sampling_gpu.py, test_cofold_sampling_gpu.py: the free energies a sampling call returns


def _rng(name):
    return np.random.default_rng([SEED] + [ord(c) for c in name])


def _batch(rng, R, L):
    """R - 1 random ACGU sequences and one of G and C only"""
    return [ppr.rand_seq(rng, L) for _ in range(R - 1)] + [ppr.rand_seq(rng, L, "GC")]


def _pairs(rng, R, la, lb):
    """R - 1 pairs over ACGU and one over G and C, each with a planted duplex across the strands"""
    return [ppr.two_strand_case(rng, la, lb, "ACGU", True) for _ in range(R - 1)] + [ppr.two_strand_case(rng, la, lb, "GC", True)]


def _ragged(rng, lens, gc):
    return [ppr.rand_seq(rng, n, "GC" if k == gc else "ACGU") for k, n in enumerate(lens)]


def _joins(db, cut):
    return any(i <= cut < j for i, j in ppr.pairs_of(db))


def _lines(strings):
    return "\n".join(strings)


def _e2(e12):
    """the second-best energy as -nd on takes it: 0 if there is none within 49 kcal/mol"""
    return e12[1] if e12[1] < INF_E and e12[1] - e12[0] <= 4900 else 0


class Op:
    """name; seqs: the sequences of the call; fields: the names of the result's entries; entry: the C entry point; takes_targets:
    the call reads installed targets (uniform or ragged)"""

    def __init__(self, name, entry, seqs, fields, install, call, reference, anchor, path=None, takes_targets=False, counters=()):
        self.name, self.entry, self.seqs, self.fields = name, entry, list(seqs), tuple(fields)
        self.install, self.call, self._reference, self._anchor, self._path = install, call, reference, anchor, path
        self.takes_targets, self.counters = takes_targets, tuple(counters)
        self._ref = None

    def run(self, engine):
        self.install(engine)
        return self.run_installed(engine)

    def run_installed(self, engine, seqs=None):
        """the call alone, with the path assertion when the sequences are the operation's own"""
        before = {c: engine.get_option(c) for c in self.counters}
        out = self.call(engine, self.seqs if seqs is None else seqs)
        if seqs is None and self._path is not None:
            self._path(engine, before)
        assert len(out) == len(self.fields), self.name
        return out

    def reference(self, oracle):
        if self._ref is None:
            self._ref = self._reference(oracle)
        return self._ref

    def anchor(self, oracle, result):
        self._anchor(self.reference(oracle), oracle, dict(zip(self.fields, result)))

    def __repr__(self):
        return "Op(%s)" % self.name


def first_difference(op, a, b):
    """name of the first field in which two results of `op` differ in any bit (None: they are the same)"""
    for name, x, y in zip(op.fields, a, b):
        if isinstance(x, np.ndarray):
            if not (isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()):
                return name
        elif x != y:
            return name
    return None


def _delta(counter, want):
    def path(e, before):
        got = e.get_option(counter) - before[counter]
        assert got == want, "%s grew by %d, the inputs were chosen for %d" % (counter, got, want)
    return path


# ---------------------------------------------------------------- score

def _score_op(name, L, R, pk=False, fused=True, workgroups=None):
    from desirna_amd import engine as E
    seqs = _batch(_rng(name), R, L)
    targets = [ppr.nested_target(L), ppr.nested_target(L, k=3)]
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL | (E.NEED_PK if pk else 0)

    def call(e, s):
        out = e.score_batch(s, flags)
        return out["Epf"], out["Emfe"], _lines(out["mfe_ss"]), out["Ed"]

    def path(e, before):
        wg = e.get_option("last_workgroups")
        assert e.get_option("last_fused") == int(fused), (name, "fused launch")
        if workgroups is not None:
            assert wg == workgroups, (name, wg)
        else:                                   # strips: R S workgroups per fold, S >= 2
            assert wg % (2 * R) == 0 and wg // (2 * R) >= 2, (name, wg)

    def reference(o):
        Epf, Emfe, ss, Ed = o.score_batch(seqs, targets)
        assert any("(" in x for x in ss) and np.isfinite(Epf).all()
        return dict(Epf=Epf, Emfe=Emfe, ss=[o.pk_struct(s, x) for s, x in zip(seqs, ss)] if pk else list(ss), Ed=Ed)

    def anchor(ref, o, got):                    # tests/test_fused_tail_gpu.py: Emfe, strings, E(target) exact, Epf within 1e-9
        assert got["mfe_ss"] == _lines(ref["ss"]) and (got["Emfe"] == ref["Emfe"]).all() and (got["Ed"] == ref["Ed"]).all()
        assert np.abs(got["Epf"] - ref["Epf"]).max() < EPF_TOL

    return Op(name, "drna_score_batch", seqs, ("Epf", "Emfe", "mfe_ss", "Ed"), lambda e: e.set_targets(targets), call, reference,
              anchor, path, takes_targets=True)


RAGGED_LENS = (12, 36, 40, 41, 79, 80, 125, 200, 201, 260)


def _score_ragged_op():
    name = "score_ragged"
    seqs = _ragged(_rng(name), RAGGED_LENS, 1)
    targets = [ppr.nested_target(n) for n in RAGGED_LENS]
    tof = list(range(len(seqs)))

    def call(e, s):
        out = e.score_ragged(s, tof)
        return out["Epf"], out["Emfe"], _lines(out["mfe_ss"]), out["Ed"]

    def reference(o):
        mfe = [o.mfe(s) for s in seqs]
        assert any("(" in ss for ss, _ in mfe)
        return dict(Epf=np.array([o.pf(s) for s in seqs]), Emfe=np.array([x for _, x in mfe]), ss=[ss for ss, _ in mfe],
                    Ed=np.array([o.eval_structure(s, t) for s, t in zip(seqs, targets)]))

    def anchor(ref, o, got):                    # tests/test_gpu_parity.py, the ragged batches: as for the uniform score
        assert got["mfe_ss"] == _lines(ref["ss"]) and (got["Emfe"] == ref["Emfe"]).all() and (got["Ed"] == ref["Ed"]).all()
        assert np.abs(got["Epf"] - ref["Epf"]).max() < EPF_TOL

    return Op(name, "drna_score_ragged", seqs, ("Epf", "Emfe", "mfe_ss", "Ed"), lambda e: e.set_targets_ragged(targets), call,
              reference, anchor, takes_targets=True)


# ---------------------------------------------------------------- two strands

def _cofold_op(name, la, lb, R=5):
    seqs = _pairs(_rng(name), R, la, lb)
    target = ppr.nested_target(la + lb, cut=la)

    def call(e, s):
        out = e.cofold_batch(s)
        return out["FA"].copy(), out["FB"].copy(), out["FcAB"].copy(), out["FAB"].copy(), out["Emfe"], _lines(out["mfe_ss"]), out["Ed"]

    def reference(o):
        mfe = [o.cofold_mfe(s) for s in seqs]
        assert any(_joins(ss, la) for ss, _ in mfe)
        return dict(F4=np.array([o.cofold_pf(s) for s in seqs]), Emfe=np.array([x for _, x in mfe]), ss=[ss for ss, _ in mfe],
                    Ed=np.array([[o.eval_structure(s, target, la)] for s in seqs]))

    def anchor(ref, o, got):                    # tests/test_cofold_native_gpu.py: EPF_TOL_ORACLE; Emfe, strings and E(target) exact
        F4 = np.stack([got[k] for k in ("FA", "FB", "FcAB", "FAB")], axis=1)
        assert np.abs(F4 - ref["F4"]).max() < EPF_TOL
        assert got["mfe_ss"] == _lines(ref["ss"]) and (got["Emfe"] == ref["Emfe"]).all() and (got["Ed"] == ref["Ed"]).all()

    return Op(name, "drna_cofold_batch", seqs, ("FA", "FB", "FcAB", "FAB", "Emfe", "mfe_ss", "Ed"), lambda e: e.set_targets([target]),
              call, reference, anchor, takes_targets=True)


def _self_dimer_op(name, L, R=6):
    seqs = _batch(_rng(name), R, L)

    def call(e, s):
        out = e.self_dimer(s)
        return out["FA"].copy(), out["FcAA"].copy(), out["FAA"].copy(), out["oligo_fraction"]

    def reference(o):
        assert any(_joins(o.cofold_mfe(s + "&" + s)[0], L) for s in seqs)
        return np.array([o.cofold_pf(s + "&" + s) for s in seqs])

    def anchor(ref, o, got):                    # tests/test_self_dimer_gpu.py: F4_TOL on FA, FcAA, FAA
        S = np.stack([got["FA"], got["FcAA"], got["FAA"]], axis=1)
        assert np.abs(S - ref[:, (0, 2, 3)]).max() < EPF_TOL

    return Op(name, "drna_self_dimer_batch", seqs, ("FA", "FcAA", "FAA", "oligo_fraction"), lambda e: None, call, reference, anchor)


# ---------------------------------------------------------------- ensemble defect

def _edef_op(name, L, lds, R=4):
    seqs = _batch(_rng(name), R, L)
    target = ppr.nested_target(L)

    def call(e, s):
        return e.ensemble_defect(s, want_bpp=True)

    def reference(o):
        ref = [o.ensemble_defect(s, target, want_bpp=True) for s in seqs]
        assert max(P.max() for _, P in ref) > 1e-3
        return np.array([d for d, _ in ref]), np.array([P for _, P in ref])

    def anchor(ref, o, got):                    # tests/test_edef_lds_gpu.py: EDEF_TOL on the defect and on every probability
        assert np.abs(got["edef"] - ref[0]).max() < EDEF_TOL and np.abs(got["bpp"] - ref[1]).max() < EDEF_TOL

    return Op(name, "drna_ensemble_defect_batch", seqs, ("edef", "bpp"), lambda e: e.set_targets([target]), call, reference, anchor,
              _delta("edef_lds_calls", int(lds)), takes_targets=True, counters=("edef_lds_calls",))


EDEF_RAGGED_LENS = (20, 36, 40, 41, 60, 120)


def _edef_ragged_op():
    name = "edef_ragged"
    seqs = _ragged(_rng(name), EDEF_RAGGED_LENS, 2)
    targets = [ppr.nested_target(n) for n in EDEF_RAGGED_LENS]
    tof = list(range(len(seqs)))

    def reference(o):
        ref = [o.ensemble_defect(s, t, want_bpp=True) for s, t in zip(seqs, targets)]
        assert max(P.max() for _, P in ref) > 1e-3
        return np.array([d for d, _ in ref])

    def anchor(ref, o, got):                    # tests/test_pair_prob_reference_gpu.py, the ragged entry point: EDEF_TOL
        assert np.abs(got["edef"] - ref).max() < EDEF_TOL

    return Op(name, "drna_ensemble_defect_ragged", seqs, ("edef",), lambda e: e.set_targets_ragged(targets),
              lambda e, s: (e.ensemble_defect_ragged(s, tof),), reference, anchor, _delta("edef_lds_calls", 1), takes_targets=True,
              counters=("edef_lds_calls",))


def _cofold_edef_op(name, la, lb, lds, R=4):
    seqs = _pairs(_rng(name), R, la, lb)
    target = ppr.nested_target(la + lb, cut=la)

    def reference(o):
        joining = max(ppr.reference_entries(o, s, [p for p in ppr.pairs_of(o.cofold_mfe(s)[0]) if p[0] <= la < p[1]] or [(1, la + lb)]).max()
                      for s in seqs)
        assert joining > 1e-3
        return np.array([ppr.reference_defect(o, s, target) for s in seqs])

    def anchor(ref, o, got):                    # tests/test_pair_prob_reference_gpu.py: EDEF_TOL against the forbidden-pair free energies
        assert np.abs(got["edef"] - ref).max() < EDEF_TOL
        P = got["bpp"]
        assert P.min() >= 0.0 and P.max() <= 1.0 and P[:, 1:la + 1, la + 1:].max() > 1e-3

    return Op(name, "drna_cofold_ensemble_defect_batch", seqs, ("edef", "bpp"), lambda e: e.set_targets([target]),
              lambda e, s: e.cofold_ensemble_defect(s, want_bpp=True), reference, anchor, _delta("edef_lds_calls", int(lds)),
              takes_targets=True, counters=("edef_lds_calls",))


class _Hip:
    """the HIP runtime calls a device entry point needs around it, taken from the runtime the engine's library is linked to
    (tests/test_fused_tail_gpu.py)"""

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


def _edef_device_op():
    """Engine.ensemble_defect_device: the caller's device buffers, made and freed in the call"""
    name = "edef_device_L120"
    L, R = 120, 4
    seqs = _batch(_rng(name), R, L)
    target = ppr.nested_target(L)

    def call(e, s):
        hip = _Hip(e._L)
        n = len(s[0])
        host = [np.frombuffer("".join(s).encode(), dtype=np.uint8).copy(), np.zeros(len(s)), np.zeros((len(s), n + 1, n + 1))]
        dev = [hip.upload(a) for a in host]                     # (the outside pass writes the pairs only: bpp goes up as zeros)
        try:
            assert hip.L.hipDeviceSynchronize() == 0
            e.ensemble_defect_device(dev[0], len(s), n, dev[1], dev[2])
            assert hip.L.hipDeviceSynchronize() == 0
            ed, bpp = hip.download(dev[1], host[1]), hip.download(dev[2], host[2])
        finally:
            for p in dev:
                hip.L.hipFree(p)
        return ed, bpp

    def reference(o):
        ref = [o.ensemble_defect(s, target, want_bpp=True) for s in seqs]
        assert max(P.max() for _, P in ref) > 1e-3
        return np.array([d for d, _ in ref]), np.array([P for _, P in ref])

    def anchor(ref, o, got):                    # as the host-buffer entry point: EDEF_TOL
        assert np.abs(got["edef"] - ref[0]).max() < EDEF_TOL and np.abs(got["bpp"] - ref[1]).max() < EDEF_TOL

    return Op(name, "drna_ensemble_defect_batch_device", seqs, ("edef", "bpp"), lambda e: e.set_targets([target]), call, reference,
              anchor, _delta("edef_lds_calls", 0), takes_targets=True, counters=("edef_lds_calls",))


# ---------------------------------------------------------------- second-best energies, ranked structures

def _subopt_op(name, L, R=4):
    seqs = _batch(_rng(name), R, L)

    def reference(o):
        assert any("(" in o.mfe(s)[0] for s in seqs)
        return np.array([o.subopt_energy(s) for s in seqs]), np.array([o.two_best(s) for s in seqs])

    def anchor(ref, o, got):                    # tests/test_gpu_parity.py::test_subopt_energy_vs_oracle: exact
        assert (got["E2"] == ref[0]).all() and (got["E12"] == ref[1]).all()

    return Op(name, "drna_subopt_energy_batch", seqs, ("E2", "E12"), lambda e: None, lambda e, s: e.subopt_energy(s, want_both=True),
              reference, anchor)


SUBOPT_RAGGED_LENS = (30, 60, 79, 80, 120, 150)


def _subopt_ragged_op():
    name = "subopt_ragged"
    seqs = _ragged(_rng(name), SUBOPT_RAGGED_LENS, 1)

    def reference(o):
        assert any("(" in o.mfe(s)[0] for s in seqs)
        return np.array([o.subopt_energy(s) for s in seqs]), np.array([o.two_best(s) for s in seqs])

    def anchor(ref, o, got):                    # tests/test_puzzle_set_aux_gpu.py: the uniform call's values, i.e. the oracle's, exact
        assert (got["E2"] == ref[0]).all() and (got["E12"] == ref[1]).all()

    return Op(name, "drna_subopt_energy_ragged", seqs, ("E2", "E12"), lambda e: None,
              lambda e, s: e.subopt_energy_ragged(s, want_both=True), reference, anchor)


def _cofold_subopt_op(name, la, lb, R=4):
    seqs = _pairs(_rng(name), R, la, lb)

    def reference(o):
        assert any(_joins(o.cofold_mfe(s)[0], la) for s in seqs)
        return [o.kbest_energies(s, 2) for s in seqs]

    def anchor(ref, o, got):                    # tests/test_kbest_reference_gpu.py: the oracle's K = 2 fill, exact
        assert [[int(x) for x in row] for row in got["E12"]] == ref and [int(x) for x in got["E2"]] == [_e2(w) for w in ref]

    return Op(name, "drna_cofold_subopt_energy_batch", seqs, ("E2", "E12"), lambda e: None,
              lambda e, s: e.cofold_subopt_energy(s, want_both=True), reference, anchor)


def _structs_op(name, K, L=None, la=None, lb=None, R=3):
    two = L is None
    seqs = _pairs(_rng(name), R, la, lb) if two else _batch(_rng(name), R, L)
    cut = la if two else 0

    def call(e, s):
        E, ss = (e.cofold_subopt_structs if two else e.subopt_structs)(s, K)
        return E, _lines(x for row in ss for x in row)

    def reference(o):
        ref = [o.kbest_energies(s, K) for s in seqs]
        assert any(row[0] < 0 for row in ref)             # a ground state with pairs
        return ref

    def anchor(ref, o, got):                    # tests/test_gpu_parity.py, test_cofold_kbest_gpu.py: every rank exact, every string re-evaluated
        assert [[int(x) for x in row] for row in got["E"]] == ref
        ss = got["ss"].split("\n")
        for r, s in enumerate(seqs):
            for k in range(K):
                if ref[r][k] < INF_E:
                    assert o.eval_structure(s, ss[r * K + k], cut) == ref[r][k], (s, k)

    return Op(name, "drna_cofold_subopt_structs_batch" if two else "drna_subopt_structs_batch", seqs, ("E", "ss"), lambda e: None, call,
              reference, anchor)


# ---------------------------------------------------------------- sampling, MEA

def _sample_op(name, S=64, L=None, la=None, lb=None, R=3):
    two = L is None
    seqs = _pairs(_rng(name), R, la, lb) if two else _batch(_rng(name), R, L)
    cut = la if two else 0
    counter = "cofold_sample_calls" if two else "sample_calls"

    def call(e, s):
        ss, E, F = (e.cofold_sample_structures if two else e.sample_structures)(s, S, seed=11)
        return _lines(x for row in ss for x in row), E, F

    def reference(o):
        if two:
            assert any(_joins(o.cofold_mfe(s)[0], la) for s in seqs)
            return np.array([o.cofold_pf(s) for s in seqs])
        assert any("(" in o.mfe(s)[0] for s in seqs)
        return np.array([o.pf(s) for s in seqs])

    def anchor(ref, o, got):                    # tests/test_sampling_gpu.py, test_cofold_sampling_gpu.py: every string re-evaluated, F within 1e-6
        assert np.abs(got["F"] - ref).max() < SAMPLE_EPF_TOL
        ss = got["ss"].split("\n")
        assert len(set(ss)) > R                                   # a sampled ensemble, not one structure per sequence
        for r, s in enumerate(seqs):
            row = ss[r * S:(r + 1) * S]
            for x in set(row):
                assert int(got["E"][r, row.index(x)]) == o.eval_structure(s, x, cut), (s, x)

    return Op(name, "drna_cofold_sample_structures_batch" if two else "drna_sample_structures_batch", seqs, ("ss", "E", "F"),
              lambda e: None, call, reference, anchor, _delta(counter, 1), counters=(counter,))


def _mea_op(name, L=None, la=None, lb=None, R=3):
    two = L is None
    seqs = _pairs(_rng(name), R, la, lb) if two else _batch(_rng(name), R, L)
    cut = la if two else 0

    def call(e, s):
        out = (e.cofold_mea_structures if two else e.mea_structures)(s, 1.0, want_bpp=True)
        return _lines(out["mea"]), out["mea_value"], _lines(out["centroid"]), out["centroid_distance"], out["E"], out["bpp"]

    def reference(o):
        if two:
            assert any(_joins(o.cofold_mfe(s)[0], la) for s in seqs)
            return None
        P = np.array([o.ensemble_defect(s, "." * L, want_bpp=True)[1] for s in seqs])
        assert P.max() > 1e-3
        return P

    def anchor(ref, o, got):                    # tests/test_mea_gpu.py: E of both strings exact; one strand: the oracle's matrix within 1e-10
        mea, cen = got["mea"].split("\n"), got["centroid"].split("\n")
        assert any("(" in x for x in mea)
        for r, s in enumerate(seqs):
            assert [int(x) for x in got["E"][r]] == [o.eval_structure(s, mea[r], cut), o.eval_structure(s, cen[r], cut)], s
        if two:
            assert got["bpp"][:, 1:la + 1, la + 1:].max() > 1e-3
        else:
            assert np.abs(got["bpp"] - ref).max() < EDEF_TOL

    return Op(name, "drna_cofold_mea_structures_batch" if two else "drna_mea_structures_batch", seqs,
              ("mea", "mea_value", "centroid", "centroid_distance", "E", "bpp"), lambda e: None, call, reference, anchor,
              _delta("mea_calls", 1), counters=("mea_calls",))


# ---------------------------------------------------------------- accessibility

def _access_op(name, L, lds, R=4):
    seqs = _batch(_rng(name), R, L)
    pos = (L // 3, 2 * L // 3)                 # 1-based: mask 0 frees nothing, masks 1 and 2 one position each

    def call(e, s):
        n = len(s[0])
        masks = np.zeros((3, n), dtype=np.uint8)
        for m, p in enumerate(pos, 1):
            masks[m, p - 1] = 1
        return (e.unpaired_free_energy(s, masks),)

    def reference(o):
        F = np.array([[o.pf(s)] + list(o.pf_forbid(s, list(pos), 0)) for s in seqs])
        assert (F[:, 1:] - F[:, :1]).max() > 0.1             # tests/access_ref.py MIN_EOPEN: a mask that costs something
        return F

    def anchor(ref, o, got):                    # tests/test_access_gpu.py: TOL = 1e-9 against the masked fill
        assert np.abs(got["F"] - ref).max() <= EPF_TOL

    return Op(name, "drna_pf_unpaired_batch", seqs, ("F",), lambda e: None, call, reference, anchor,
              _delta("access_lds_calls", int(lds)), counters=("access_lds_calls",))


# ---------------------------------------------------------------- native Monte-Carlo loops

MC_R, MC_ITER = 4, 20
MC_FIELDS = ("seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed", "counters", "best_seq", "best_ss", "best_vals", "rng")
START_SCORE = 1e3                 # above any score a fold gives: every chain takes its first proposal


def _mc_start(rows, dots, extra=()):
    """the state arrays of a loop that starts from the sequences `rows` with nothing folded yet"""
    C = len(rows)
    state = dict(seqs=np.frombuffer("".join(rows).encode(), np.uint8).copy(), mfe_ss=np.frombuffer("".join(dots).encode(), np.uint8).copy(),
                 score=np.full(C, START_SCORE), mcc1=np.ones(C), Epf=np.zeros(C), Ed=np.zeros(C))
    for k in extra:
        state[k] = np.zeros(C)
    return state


def _mc_result(state, counters, best, rng):
    return tuple(state[k] for k in MC_FIELDS[:6]) + (counters, best["seq"], best["ss"], best["vals"], rng)


def _mc_anchor(lens, amp):
    def anchor(ref, o, got):                    # tests/test_cofold_native_gpu.py: EPF_TOL_ORACLE; the structures exact
        assert got["counters"].reshape(-1, 3)[:, 0].all()                      # every problem moved
        flat, ss, off = got["seqs"].tobytes().decode(), got["mfe_ss"].tobytes().decode(), 0
        for c, n in enumerate(lens):
            s, x = flat[off:off + n], ss[off:off + n]
            off += n
            if amp:
                db, _ = o.cofold_mfe(s)
                assert x == db and abs(got["Epf"][c] - o.cofold_pf(s)[3]) < EPF_TOL, s
            else:
                assert x == o.mfe(s)[0] and abs(got["Epf"][c] - o.pf(s)) < EPF_TOL, s
    return anchor


def _mc_reference(probs, rows):
    def reference(o):
        for p in probs:
            assert "(" in p.sec_struct
        for s in rows:                          # the oracle folds every start sequence
            assert ("&" in s) == ("&" in probs[0].sec_struct) and set(s) <= set("ACGU&")
            assert np.isfinite(o.cofold_pf(s)[3] if "&" in s else o.pf(s))
        return None
    return reference


def _mc_run_op():
    from desirna_amd import design, engine as E
    prob = design.DesignProblem(TARGET36)
    rows = [prob.initial_sequence(random.Random(SEED + c)) for c in range(MC_R)]
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL

    def call(e, s):
        n = len(s[0])
        state = _mc_start(s, ["." * n] * len(s))
        for k in ("seqs", "mfe_ss"):
            state[k] = state[k].reshape(len(s), n)
        best = dict(seq=state["seqs"][0].copy(), ss=state["mfe_ss"][0].copy(), vals=np.array([2.0, 0.0, 0.0, 0.0]))
        counters, rng = np.zeros(3, np.int64), E.HostKernels().rng_seed(np.arange(len(s)))
        e.mc_run(prob, MC_ITER, np.arange(len(s), dtype=np.int32), len(s), 0.7, 0.0, True, np.linspace(10, 150, len(s)),
                 [("Ed-Epf", 1.0)], flags, rng, state, counters, best)
        return _mc_result(state, counters, best, rng)

    return Op("mc_run", "drna_mc_run", rows, MC_FIELDS, lambda e: e.set_targets([TARGET36]), call, _mc_reference([prob], rows),
              _mc_anchor([36] * MC_R, False), takes_targets=True)


def _mc_run_cofold_op():
    from desirna_amd import design, engine as E
    prob = design.DesignProblem(CO_TARGET37, "N" * 18 + "&" + "N" * 18)            # (the restraint string carries the '&' too)
    cut = CO_TARGET37.index("&")
    rows = [prob.initial_sequence(random.Random(SEED + 10 + c)) for c in range(MC_R)]

    def call(e, s):
        n = len(s[0])
        state = _mc_start(s, ["." * cut + "&" + "." * (n - cut - 1)] * len(s), extra=("oligo_fraction", "bonus"))
        for k in ("seqs", "mfe_ss"):
            state[k] = state[k].reshape(len(s), n)
        best = dict(seq=state["seqs"][0].copy(), ss=state["mfe_ss"][0].copy(), vals=np.zeros(6))
        best["vals"][0] = 2.0
        counters, rng = np.zeros(3, np.int64), E.HostKernels().rng_seed(np.arange(len(s)))
        e.mc_run_cofold(prob, "heterodimer", MC_ITER, np.arange(len(s), dtype=np.int32), len(s), 0.7, 0.0, True,
                        np.linspace(10, 150, len(s)), [("Ed-Epf", 1.0)], rng, state, counters, best)
        return _mc_result(state, counters, best, rng) + (state["oligo_fraction"], state["bonus"])

    return Op("mc_run_cofold", "drna_mc_run_cofold", rows, MC_FIELDS + ("oligo_fraction", "bonus"),
              lambda e: e.set_targets([CO_TARGET37.replace("&", "")]), call, _mc_reference([prob], rows), _mc_anchor([37] * MC_R, True),
              takes_targets=True)


def _mc_run_ragged_op():
    from desirna_amd import design, engine as E
    probs = [design.DesignProblem(TARGET12), design.DesignProblem(TARGET36)]
    Rs = [2, 2]
    rows = [p.initial_sequence(random.Random(SEED + 20 + 10 * k + c)) for k, (p, R) in enumerate(zip(probs, Rs)) for c in range(R)]
    flags = E.NEED_PF | E.NEED_MFE | E.NEED_EVAL

    def call(e, s):
        state = _mc_start(s, ["." * len(x) for x in s])
        firsts = [s[0], s[Rs[0]]]
        best = dict(seq=np.frombuffer("".join(firsts).encode(), np.uint8).copy(),
                    ss=np.frombuffer("".join("." * len(x) for x in firsts).encode(), np.uint8).copy(),
                    vals=np.tile(np.array([2.0, 0.0, 0.0, 0.0]), (len(probs), 1)))
        counters, rng = np.zeros((len(probs), 3), np.int64), E.HostKernels().rng_seed(np.concatenate([np.arange(R) for R in Rs]))
        e.mc_run_ragged(probs, MC_ITER, np.concatenate([np.arange(R, dtype=np.int32) for R in Rs]), Rs, 0.7, 0.0, True,
                        np.concatenate([np.linspace(10, 150, R) for R in Rs]), [("Ed-Epf", 1.0)], flags, rng, state, counters, best)
        return _mc_result(state, counters, best, rng)

    return Op("mc_run_ragged", "drna_mc_run_ragged", rows, MC_FIELDS, lambda e: None, call, _mc_reference(probs, rows),
              _mc_anchor([12, 12, 36, 36], False), takes_targets=True)


# ---------------------------------------------------------------- the table

def build_ops():
    return [
        _score_op("score_L200_R2", 200, 2, workgroups=8),                     # before R = 9: exchange rows and flag sets grow
        _score_op("score_L200_R9", 200, 9, workgroups=36),
        _score_op("score_pk_L170_R8", 170, 8, pk=True, workgroups=32),
        _score_op("score_L36_R16", 36, 16, fused=False, workgroups=32),
        _score_op("score_L260_R3", 260, 3, fused=False),                      # strips
        _score_ragged_op(),
        _cofold_op("cofold_18_18", 18, 18),
        _cofold_op("cofold_50_50", 50, 50),
        _self_dimer_op("self_dimer_L30", 30),
        _self_dimer_op("self_dimer_L100", 100),
        _edef_op("edef_L36", 36, lds=True),
        _edef_op("edef_L120", 120, lds=False),
        _edef_ragged_op(),
        _edef_device_op(),
        _cofold_edef_op("cofold_edef_20_20", 20, 20, lds=True),
        _cofold_edef_op("cofold_edef_40_40", 40, 40, lds=False),
        _subopt_op("subopt_L60", 60),
        _subopt_op("subopt_L120", 120),
        _subopt_ragged_op(),
        _cofold_subopt_op("cofold_subopt_30_30", 30, 30),
        _cofold_subopt_op("cofold_subopt_50_50", 50, 50),
        _structs_op("structs_L60_K4", 4, L=60),
        _structs_op("structs_L100_K8", 8, L=100),
        _structs_op("cofold_structs_20_20_K4", 4, la=20, lb=20),
        _sample_op("sample_L100_S64", L=100),
        _sample_op("cofold_sample_30_30_S64", la=30, lb=30),
        _mea_op("mea_L100", L=100),
        _mea_op("mea_L200", L=200),
        _mea_op("cofold_mea_30_30", la=30, lb=30),
        _access_op("access_L30", 30, lds=True),
        _access_op("access_L100", 100, lds=False),
        _mc_run_op(),
        _mc_run_cofold_op(),
        _mc_run_ragged_op(),
    ]


OPS = build_ops()
NAMES = [op.name for op in OPS]
BY_NAME = {op.name: op for op in OPS}
NO_TARGET_OPS = [op for op in OPS if not op.takes_targets]     # second-best, ranked, sampling, MEA, accessibility, self-dimer
