"""The constructed loops of tests/constructs.py through the UNMODIFIED kernel sources on the CPU (tests/emu): the same comparison
with the oracle as tests/test_loop_constructs_gpu.py, on the shapes at both ends of the size range, so that a wrong loop shape
can be traced to a kernel -- and, through the table comparison at the end, to a cell -- without a GPU.

The emulation waits on thread rendezvous most of the time, so every (kernel, record) pair is one job of a pool of worker
processes (one job per process at a time: the emulated __shared__ is a function-local static); the tests below read the results."""
import numpy as np
import pytest

from tests import constructs as C

SIZES = (0, 1, 2, 3, 4, 6, 29, 30, 31)
EPF_TOL = 1e-9                  # kcal/mol, as in tests/test_kernels_emulated.py
INF_DEV = 1 << 22
INF_REF = 10000000


def _shapes():
    return [(u1, s - u1) for s in SIZES for u1 in sorted({0, 1, 2, s // 2}) if u1 <= s]


def _small_record(oracle, k, u1, u2):
    """the first oracle-checked filling of shape k's closing-pair combination (of the next combination that has one)"""
    for step in range(36):
        po, pi = C.PAIRS[(k + step) % 6], C.PAIRS[(k // 2 + 1 + step // 6) % 6]
        for r in C.small_candidates(u1, u2, po, pi):
            if C.has_loop(oracle.mfe(r.sequence)[0], r):
                return r
    raise AssertionError((u1, u2))


def _records(oracle):
    """28 interior shapes, one small-loop record per shape (its loop in the MFE), hairpins at both ends of the tabulated range, two
    special loops"""
    recs = [C.interior_record(u1, u2) for u1, u2 in _shapes()]
    recs += [_small_record(oracle, k, u1, u2) for k, (u1, u2) in enumerate(C.SMALL_SHAPES)]
    hp = {r.name: r for r in C.hairpin()}
    recs += [hp["hp_%d" % h] for h in (3, 4, 30, 31, 45)]
    recs += [hp["hp_special_" + e] for e in (C.special_hairpins()[0], C.special_hairpins()[-1])]
    return recs


STRIP_SHAPES = ((15, 15, 40), (0, 30, 40), (15, 16, 12))       # (u1, u2, left offset in the 100-nt frame)
_emus = {}


def _emu(kind, params_name="turner1999"):
    """this process's emulator of one kind on one parameter set of tests/probe_params.py (built once per process)"""
    if (kind, params_name) not in _emus:
        from tests.probe_params import probe_blob
        blob = probe_blob(params_name)
        if kind == "emu":
            from tests.emu.emu import Emu
            _emus[kind, params_name] = Emu(blob)
        elif kind == "co_lds":
            from tests.emu.emu_cofold_lds import EmuCofoldLds
            _emus[kind, params_name] = EmuCofoldLds(blob)
        else:
            from tests.emu.emu_self_dimer import EmuSelfDimer
            _emus[kind, params_name] = EmuSelfDimer(blob)
    return _emus[kind, params_name]


def _job(job, params_name="turner1999"):
    """(kind, sequence[, target]) -> plain Python values; runs in a worker process"""
    kind, s = job[0], job[1]
    if kind in ("gen", "lds"):
        nt = 128 if kind == "gen" else -256
        E, ss, st = _emu("emu", params_name).mfe([s], nt=nt)
        Ep, stp = _emu("emu", params_name).pf([s], nt=nt)
        return int(E[0]), ss[0], float(Ep[0]), int(st[0]), int(stp[0])
    if kind == "dual":
        E, ss, st = _emu("emu", params_name).mfe_dual([s], nt=256)
        return int(E[0]), ss[0], int(st[0])
    if kind == "subopt":
        E2, E12, st = _emu("emu", params_name).subopt([s], nt=64)
        return int(E2[0]), (int(E12[0, 0]), int(E12[0, 1])), int(st[0])
    if kind == "co_gen":
        E, ss, F4, st, Ed = _emu("emu", params_name).cofold([s], job[2], nt=64)
        return int(E[0]), ss[0], [float(x) for x in F4[0]], [int(x) for x in st], int(Ed[0])
    if kind == "co_lds":
        E, ss, F4, st = _emu("co_lds", params_name).cofold([s], nt=128)
        return int(E[0]), ss[0], [float(x) for x in F4[0]], [int(x) for x in st]
    if kind == "sd":
        out = []
        for lds in (True, False):
            F4, st = _emu("sd", params_name).fold([s], nt=128, lds=lds)
            out.append(([float(x) for x in F4[0]], int(st[0])))
        return out
    assert kind == "strip"
    E, ss, st = _emu("emu", params_name).mfe_strip([s], 2, nt=256)
    Ep, stp = _emu("emu", params_name).pf_strip([s], 2, nt=256)
    return int(E[0]), ss[0], float(Ep[0]), int(st[0]), int(stp[0])


def _selfdimer_records():
    return [C.selfdimer()[u] for u in (0, 7, 15, 16)]           # loop sizes 0, 14, 30 and 32 (up to 44 nt: the LDS kernel's range)


def _strip_frames():
    return [C.pad(C.interior_record(u1, u2), 100, offset=off) for u1, u2, off in STRIP_SHAPES]


@pytest.fixture(scope="module")
def results(oracle):
    from tests.emu.emu import _spawn_map
    for kind in ("emu", "co_lds", "sd"):
        _emu(kind)                                          # compile before the workers load the libraries
    jobs = [("strip", f[0]) for f in _strip_frames()]       # longest jobs first
    jobs += [("subopt", r.sequence) for r in sorted(_records(oracle), key=lambda r: -len(r.sequence))]
    for u1, u2 in _shapes():
        r = C.cofold_record(u1, u2)
        jobs += [("co_gen", r.sequence, r.target), ("co_lds", r.sequence)]
    jobs += [("sd", r.sequence) for r in _selfdimer_records()]
    jobs += [(kind, r.sequence) for kind in ("dual", "lds", "gen") for r in _records(oracle)]
    return dict(zip(jobs, _spawn_map(_job, jobs, 16)))


def test_record_set(oracle):
    recs = _records(oracle)
    assert len(_shapes()) == 28 and len(recs) == 28 + 12 + 5 + 2 and max(len(r.sequence) for r in recs) <= 64
    hits = [r for r in recs if C.has_loop(oracle.mfe(r.sequence)[0], r)]
    assert len([r for r in hits if r.family == "interior"]) == 24 and len([r for r in hits if r.family == "hairpin"]) == 7
    assert len([r for r in hits if r.family == "small"]) == 12 and len({C.shape_of(r) for r in hits if r.family == "small"}) == 12


@pytest.mark.parametrize("kind", ["gen", "lds"])
def test_mfe_and_pf_kernels(results, oracle, kind):
    """general kernels (128 threads) and LDS-resident kernels (256 threads)"""
    for r in _records(oracle):
        E, ss, Ep, st, stp = results[(kind, r.sequence)]
        assert (st, stp) == (0, 0), r.name
        assert (ss, E) == oracle.mfe(r.sequence), (kind, r.name)
        assert abs(Ep - oracle.pf(r.sequence)) < EPF_TOL, (kind, r.name)


def test_two_workgroup_mfe_kernel(results, oracle):
    for r in _records(oracle):
        E, ss, st = results[("dual", r.sequence)]
        assert st == 0 and (ss, E) == oracle.mfe(r.sequence), r.name


def test_second_best_kernel(results, oracle):
    for r in _records(oracle):
        E2, E12, st = results[("subopt", r.sequence)]
        assert st == 0 and E12 == oracle.two_best(r.sequence), r.name
        assert E2 == oracle.subopt_energy(r.sequence) and E12[0] == oracle.mfe(r.sequence)[1], r.name
    for u1, u2, inside in ((14, 15, True), (15, 15, True), (15, 16, False)):
        r = C.interior_record(u1, u2)                          # up to the limit the loop structure is the best one, above it no candidate at all
        e1 = results[("subopt", r.sequence)][1][0]
        assert (e1 == oracle.eval_structure(r.sequence, r.target)) == inside and (inside or e1 == -1070), r.name


def test_cofold_kernels(results, oracle):
    """general and short-pair (LDS) co-fold kernels on the two-strand form of the 28 shapes; E(target) with the nick"""
    for u1, u2 in _shapes():
        r = C.cofold_record(u1, u2)
        oss, oe = oracle.cofold_mfe(r.sequence)
        f4 = np.array(oracle.cofold_pf(r.sequence))
        E, ss, F4, st, Ed = results[("co_gen", r.sequence, r.target)]
        assert not any(st) and (ss, E) == (oss, oe), r.name
        assert np.abs(np.array(F4) - f4).max() < EPF_TOL, r.name
        assert Ed == oracle.eval_structure(r.sequence, r.target, cut=C.cut_of(r)), r.name
        E, ss, F4, st = results[("co_lds", r.sequence)]
        assert not any(st) and (ss, E) == (oss, oe), r.name
        assert np.abs(np.array(F4) - f4).max() < EPF_TOL, r.name
        assert (ss == r.target) == (u1 + u2 <= C.MAXLOOP), r.name


def test_self_dimer_kernels(results, oracle):
    for r in _selfdimer_records():
        (F_lds, st_lds), (F_ws, st_ws) = results[("sd", r.sequence)]
        assert (st_lds, st_ws) == (0, 0) and F_lds == F_ws, r.name                  # bit for bit, as on the GPU
        o = oracle.cofold_pf(r.sequence + "&" + r.sequence)
        assert max(abs(F_lds[c] - o[c]) for c in (0, 2, 3)) < EPF_TOL, r.name


def test_two_strip_kernels(results, oracle):
    """mfe_strip / pf_strip with two strips of a 100-nt frame: the strips part in the 5' side of the 15 x 15 loop, under the
    inner hairpin of 0 x 30, and in the 3' side of 15 x 16"""
    for (u1, u2, _), (s, t, o), (lo, hi) in zip(STRIP_SHAPES, _strip_frames(), ((0, 2), (2, 3), (3, 1))):
        lp = C.interior_record(u1, u2).intended_loop
        assert o + lp[lo] < 47 and o + lp[hi] > 53                     # either side of column 50, whatever the rounding
        E, ss, Ep, st, stp = results[("strip", s)]
        assert (st, stp) == (0, 0)
        assert (ss, E) == oracle.mfe(s), (u1, u2)
        assert (ss == t) == (u1 + u2 <= C.MAXLOOP), (u1, u2)
        assert abs(Ep - oracle.pf(s)) < EPF_TOL, (u1, u2)


@pytest.mark.parametrize("shape", [(15, 15), (0, 30), (1, 29)])
def test_mfe_tables_match_oracle_on_constructs(blob, oracle, shape):
    """cell by cell: c and fML of the general kernel, and c of the LDS-resident kernel (it leaves no fML table behind: its
    multiloop rows live in LDS), on the padded construct.  A wrong tower slot or ring row shows up as the cell it spoiled."""
    from tests.emu.emu import Emu
    emu = Emu(blob)
    s, t, off = C.pad(C.interior_record(*shape), 60, 0)
    c, f, f5 = oracle.mfe_tables(s)
    n = len(s)
    want = lambda x: x if x < INF_REF else INF_DEV
    for nt in (128, -256):
        E, ss, st, Wc, F = emu.mfe([s], nt=nt, dump=True)
        assert (ss[0], int(E[0])) == oracle.mfe(s) and ss[0] == t
        for d in range(4, n):
            for i in range(1, n - d + 1):
                assert want(c[i, i + d]) == Wc[d, i] >> 8, (nt, i, i + d)
                if nt > 0:
                    assert want(f[i, i + d]) == F[d, i], (nt, i, i + d)
    assert c[off + 4, off + 17 + sum(shape)] < INF_REF           # the outer pair's cell (1-based) holds the loop
