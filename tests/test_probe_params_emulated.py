"""The UNMODIFIED kernel sources on the CPU (tests/emu) under the probe parameter sets of tests/probe_params.py, against the
oracle on the same blob (tests/test_probe_params_oracle.py pins that oracle to enumeration).  Turner-1999 cannot tell mmI from
mm1n, mmM from mmExt or d5 + d3, eMLb from scale, or a swapped pair of indices of stack / int11; the "distinct" probe can, on
every fold path the emulation reaches.  "full_special" fills the special-loop tables to their capacity.

Under the probe a record's loop need not be in the MFE structure any more; the evaluation of its target reads that loop's table
entry whatever the fold does, and the partition function sums it.  All emulation jobs of the module run once, side by side in
worker processes (the job carries the blob's name; a worker builds its emulators from probe_blob(name))."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import constructs as C
from tests import probe_params as PP
from tests import test_loop_constructs_emulated as LC
from tests.test_cofold_edef_emulated import EDEF_TOL, defect_from_matrix, enumerate_ensemble
from tests.test_cofold_subopt_emulated import cofold_structures
from tests.test_kernels_emulated import _all_structures

EPF_TOL = LC.EPF_TOL
INF_REF = 10000000
PKT_FLAGS, PKT_TAG = ("-DDRNA_PKT_W=6", "-DDRNA_PKT_L=3"), "_pktw6"      # the second tile-product window of test_kernels_emulated.py
SUBSET = ("small_1x3", "small_2x3", "small_1x1", "small_2x1", "small_2x2", "small_0x2", "int_1x5", "int_0x6",
          "hp_3", "hp_special_")            # name prefixes in LC._records: 1 x n, 2 x 3, 1 x 1, 2 x 1, 2 x 2, bulges, the special hairpins
HELPER_L = 64                               # the PF helper workgroup folds the subset inside 64-nt frames (256 threads cover n <= 64).
                                            # The engine gives a sequence a helper from 95 nt on; tests/test_kernels_emulated.py emulates
                                            # the pair from 30 nt on; at 22, 23 and 24 nt the emulated pair never returns, under Turner-1999 too
CO_SHAPES = ((1, 3), (2, 3), (1, 1), (2, 1), (2, 2), (0, 2))
_emus = {}


def _emu(kind, name):
    """this process's emulator of one kind on one probe (built once per process)"""
    if (kind, name) not in _emus:
        blob = PP.probe_blob(name)
        if kind == "pkt":
            from tests.emu.emu import Emu
            _emus[kind, name] = Emu(blob, flags=PKT_FLAGS, tag=PKT_TAG)
        elif kind == "subopt_lds":
            from tests.emu.emu_subopt_lds import EmuSuboptLds
            _emus[kind, name] = EmuSuboptLds(blob)
        elif kind == "edef_lds":
            from tests.emu.emu_edef_lds import EmuEdefLds
            _emus[kind, name] = EmuEdefLds(blob)
        elif kind == "kbest":
            from tests.emu.emu_cofold_kbest import EmuCofoldKbest
            _emus[kind, name] = EmuCofoldKbest(blob)
        else:
            assert kind == "ragged"
            from tests.emu.emu_ragged_aux import EmuRaggedAux
            _emus[kind, name] = EmuRaggedAux(blob)
    return _emus[kind, name]


def _job(job):
    """(blob name, kind, sequence or pair, ...) -> plain Python values; runs in a worker process.  The kinds of
    tests/test_loop_constructs_emulated.py go to its _job with the blob's name."""
    name, kind, s = job[0], job[1], job[2]
    e = LC._emu("emu", name)
    if kind == "eval":
        return [int(e.eval([x], [t])[0, 0]) for x, t in s]
    if kind == "pf_helper":
        Eh, sth = e.pf([s], nt=-257)
        E1, st1 = e.pf([s], nt=-256)
        return float(Eh[0]), float(E1[0]), int(sth[0]), int(st1[0])
    if kind == "strip":                                       # job[3]: blocked (fark splits, second tile-product window)
        E, ss, st = e.mfe_strip([s], 2, nt=256, fark=int(job[3]))
        Ep, stp = (_emu("pkt", name) if job[3] else e).pf_strip([s], 2, nt=256)
        return int(E[0]), ss[0], float(Ep[0]), int(st[0]), int(stp[0])
    if kind == "kbest":                                       # one or two strands, K = job[3]
        E, ss, st = _emu("kbest", name).kbest([s], job[3], nt=64)
        return [int(x) for x in E[0]], ss[0], int(st[0])
    if kind == "kbest_gen":                                   # kbest_kernel through libemu.so
        E, ss, st = e.kbest([s], job[3], nt=64)
        return [int(x) for x in E[0]], ss[0], int(st[0])
    if kind == "second_best":                                 # one or two strands, job[3]: the LDS kernel
        E2, E12, st = _emu("subopt_lds", name).second_best([s], lds=job[3], nt=64)
        return int(E2[0]), (int(E12[0, 0]), int(E12[0, 1])), int(st[0])
    if kind == "outside":
        ed, st, B = e.edef([s], job[3], nt=64, bpp=True)
        return float(ed[0]), B[0], int(st[0])
    if kind == "edef_lds":                                    # one or two strands
        ed, bpp, F4, st = _emu("edef_lds", name).edef([s], job[3], nt=64)
        return float(ed[0]), bpp[0], [float(x) for x in F4[0]], int(st[0])
    if kind == "co_outside":
        ed, bpp, F4, st = e.cofold_edef([s], job[3], nt=64)
        return float(ed[0]), bpp[0], [float(x) for x in F4[0]], int(st[0])
    if kind == "co_second_best":
        E2, E12, st = e.cofold_subopt([s], nt=64)
        return int(E2[0]), (int(E12[0, 0]), int(E12[0, 1])), int(st[0])
    if kind == "ragged":                                      # s: the sequences of one ragged launch; job[3]: aux kind, job[4]: targets
        order = list(range(len(s)))[::-1]
        out = _emu("ragged", name).ragged(job[3], list(s), order, list(job[4]) if job[4] else None, nt=64)
        return {k: np.asarray(v).tolist() for k, v in out.items()}
    return LC._job(job[1:], name)


# ---- the cases

def probe_records():
    """the fixed sequences of tests/probe_params.py as records: triloop, hexaloop, multiloop with unpaired bases"""
    out = []
    for nm, (s, t) in (("probe_tri", PP.TRI_HAIRPIN), ("probe_hexa", PP.HEXA_HAIRPIN)):
        out.append(C.Record(nm, "hairpin", s, t, (2, len(s) - 3)))
    s, t = PP.MULTILOOP
    out.append(C.Record("probe_multiloop", "multiloop", s, t, (1, len(s) - 2, 2)))
    return out


def extra_records(oracle):
    """what the constructed loops leave out: two pinned multiloops (stem terms of the multiloop in the ground state) and three
    random 36-mers (asymmetric 1 x 1 loops, dangles at the ends); a random sequence's target is its Turner-1999 structure"""
    rng = np.random.default_rng(36)
    out = C.multiloop()[:2]
    for k in range(3):
        s = "".join(rng.choice(list("ACGU" if k else "GGCCAU"), 36))
        out.append(C.Record("random36_%d" % k, "random", s, oracle.mfe(s)[0], (0, 35)))
    return out


def _all_records(oracle):
    """the record set of tests/test_loop_constructs_emulated.py (chosen by the Turner-1999 oracle, as there) + the probe's own"""
    return LC._records(oracle) + probe_records() + extra_records(oracle)


def _subset(oracle):
    recs = _all_records(oracle)
    out = [next(r for r in recs if r.name.startswith(p)) for p in SUBSET[:-1]]
    out += [r for r in recs if r.name.startswith(SUBSET[-1])] + probe_records()
    assert len({r.name for r in out}) == len(out) == len(SUBSET) + 1 + len(probe_records())      # (two special hairpins)
    return out


def special_frame():
    """100 nt that hold the probe's triloop and hexaloop hairpins, the multiloop with unpaired bases and a tabulated tetraloop"""
    tetra = PP.special_hairpin(PP.turner_dict()["Tetraloops"][0][0])
    parts = [PP.special_hairpin("GAAAC"), PP.special_hairpin("ACAGUACU"), PP.MULTILOOP, tetra]
    s = "AA" + "AAA".join(p[0] for p in parts)
    t = ".." + "...".join(p[1] for p in parts)
    return s + "A" * (100 - len(s)), t + "." * (100 - len(s))


def _framed(rec):
    """the record inside a 64-nt poly-A frame (the PF helper's case)"""
    return C.pad(rec, HELPER_L)[0]


def _strip_cases():
    return [(f[0], f[1]) for f in LC._strip_frames()] + [special_frame()]


def _short_pairs():
    """pairs short enough to enumerate every co-fold structure; the last one is a homodimer"""
    rng = np.random.default_rng(2026)
    out = []
    for k in range(6):
        la, lb = (int(x) for x in rng.integers(4, 8, size=2))
        alpha = ("ACGU", "GGCCAU")[k % 2]
        a = "".join(rng.choice(list(alpha), la))
        out.append(a + "&" + (a if k == 5 else "".join(rng.choice(list(alpha), lb))))
    return out


def _sharp_pairs():
    """(pair, target) for the "distinct_sharp" probe, short enough to enumerate every co-fold structure; two homodimers; the
    target is the pair's co-fold ground state under that probe, or the open chain"""
    orc = pyoracle.Oracle(PP.probe_blob("distinct_sharp"))
    rng = np.random.default_rng(2027)
    out = []
    for k in range(10):
        la, lb = (int(x) for x in rng.integers(5, 9, size=2))
        alpha = ("GGCCAU", "ACGU", "GCU")[k % 3]
        a = "".join(rng.choice(list(alpha), la))
        s = a + "&" + (a if k % 5 == 4 else "".join(rng.choice(list(alpha), lb)))
        out.append((s, orc.cofold_mfe(s)[0] if k % 2 else "." * s.index("&") + "&" + "." * (len(s) - s.index("&") - 1)))
    return out


def _co_records():
    return [C.cofold_record(u1, u2) for u1, u2 in CO_SHAPES]


def _full_special_records():
    hp = {r.name: r for r in C.hairpin()}
    recs = [hp["hp_%d" % h] for h in (3, 4, 30, 31, 45)]
    recs += [hp["hp_special_" + e] for e in (C.special_hairpins()[0], C.special_hairpins()[-1])]
    for which, lst in zip(("tri", "tetra", "hexa"), PP.special_loops("full_special")):
        for k in (0, len(lst) - 1):
            s, t = PP.special_hairpin(lst[k][0])
            recs.append(C.Record("full_%s_%d" % (which, k), "hairpin", s, t, (4, len(s) - 5)))
    return recs


RAGGED_KINDS = ("edef_lds", "edef_general", "subopt_lds", "subopt_general")


def _ragged_set(oracle):
    """four lengths of the subset in one ragged launch per auxiliary kernel"""
    sub = {r.name: r for r in _subset(oracle)}
    picks = [sub["probe_multiloop"], sub["probe_hexa"], next(r for n, r in sub.items() if n.startswith("small_2x3")),
             next(r for n, r in sub.items() if n.startswith("small_1x3"))]
    return tuple(r.sequence for r in picks), tuple(r.target for r in picks)


@pytest.fixture(scope="module")
def probe_oracle():
    pyoracle.build()
    return pyoracle.Oracle(PP.probe_blob("distinct"))


@pytest.fixture(scope="module")
def full_oracle():
    pyoracle.build()
    return pyoracle.Oracle(PP.probe_blob("full_special"))


def _jobs(oracle):
    """every emulation job of the module, the longest first"""
    D = "distinct"
    recs, sub = _all_records(oracle), _subset(oracle)
    jobs = [(D, "strip", s, b) for s, _ in _strip_cases() for b in (False, True)]          # longest jobs first
    for r in sorted(sub, key=lambda r: -len(r.sequence)):
        s, t = r.sequence, r.target
        jobs += [(D, "subopt", s), (D, "second_best", s, True), (D, "dual", s), (D, "pf_helper", _framed(r)),
                 (D, "outside", s, t), (D, "outside", s, "." * len(s)), (D, "edef_lds", s, t)]
    for k, r in enumerate(sub):                                # the ranked lists: K = 4 (kbest_kernel) and K = 8 on alternate records
        jobs.append((D, "kbest_gen", r.sequence, 4) if k % 2 else (D, "kbest", r.sequence, 8))
    for r in _co_records():
        s, t = r.sequence, r.target
        jobs += [(D, "co_gen", s, t), (D, "co_lds", s), (D, "co_second_best", s), (D, "second_best", s, True),
                 (D, "kbest", s, 4 if len(s) % 2 else 8), (D, "co_outside", s, t), (D, "edef_lds", s, t)]
    for s in _short_pairs():
        t = "." * s.index("&") + "&" + "." * (len(s) - s.index("&") - 1)
        jobs += [(D, "co_gen", s, t), (D, "co_lds", s), (D, "co_second_best", s), (D, "second_best", s, True), (D, "kbest", s, 8),
                 (D, "co_outside", s, t), (D, "edef_lds", s, t)]
    for s, t in _sharp_pairs():
        jobs += [("distinct_sharp", "co_outside", s, t), ("distinct_sharp", "edef_lds", s, t)]
    jobs += [(D, "sd", r.sequence) for r in LC._selfdimer_records()]
    seqs, tgts = _ragged_set(oracle)
    jobs += [(D, "ragged", seqs, kind, tgts if kind.startswith("edef") else None) for kind in RAGGED_KINDS]
    jobs += [(D, kind, r.sequence) for kind in ("lds", "gen") for r in recs]
    jobs += [(D, "eval", tuple((r.sequence, r.target) for r in recs))]
    full = _full_special_records()
    jobs += [("full_special", kind, r.sequence) for kind in ("lds", "gen") for r in full]
    jobs += [("full_special", "eval", tuple((r.sequence, r.target) for r in full))]
    return jobs


@pytest.fixture(scope="module")
def results(oracle):
    from tests.emu import emu, emu_cofold_kbest, emu_cofold_lds, emu_edef_lds, emu_ragged_aux, emu_self_dimer, emu_subopt_lds
    emu.build()
    emu.build(PKT_FLAGS, PKT_TAG)                              # compile before the workers load the libraries
    for m in (emu_cofold_kbest, emu_cofold_lds, emu_edef_lds, emu_ragged_aux, emu_self_dimer, emu_subopt_lds):
        m.build()
    jobs = _jobs(oracle)
    return dict(zip(jobs, emu._spawn_map(_job, jobs, 16)))


# ---- one strand

def test_case_set(oracle, probe_oracle):
    sub = _subset(oracle)
    shapes = {C.shape_of(r) for r in sub if len(r.intended_loop) == 4}
    assert {(1, 3), (2, 3), (1, 1), (2, 1), (2, 2), (0, 2), (1, 5), (0, 6)} <= shapes
    assert len(_all_records(oracle)) == len(LC._records(oracle)) + 3 + 5 and max(len(r.sequence) for r in sub) <= 64
    s, t = special_frame()
    assert len(s) == len(t) == 100 and probe_oracle.eval_structure(s, t) < 0
    # the probe's special hairpins are the ground state of their fixed sequences, so the folds' tracebacks read them; the short
    # multiloop is not (MLclosing = 310): its terms are read by the evaluation of its target and summed by the partition function
    for r in probe_records()[:2]:
        assert C.has_loop(probe_oracle.mfe(r.sequence)[0], r), r.name
    assert probe_oracle.eval_structure(*PP.MULTILOOP) < INF_REF


@pytest.mark.parametrize("kind", ["gen", "lds"])
def test_mfe_and_pf_kernels(results, oracle, probe_oracle, kind):
    """general kernels (128 threads) and LDS-resident kernels (256 threads), the full record set"""
    for r in _all_records(oracle):
        E, ss, Ep, st, stp = results[("distinct", kind, r.sequence)]
        assert (st, stp) == (0, 0), r.name
        assert (ss, E) == probe_oracle.mfe(r.sequence), (kind, r.name)
        assert abs(Ep - probe_oracle.pf(r.sequence)) < EPF_TOL, (kind, r.name)


def test_eval_kernel_on_every_target(results, oracle, probe_oracle):
    recs = _all_records(oracle)
    got = results[("distinct", "eval", tuple((r.sequence, r.target) for r in recs))]
    for r, e in zip(recs, got):
        assert e == probe_oracle.eval_structure(r.sequence, r.target), r.name


def test_two_workgroup_mfe_and_pf_helper(results, oracle, probe_oracle):
    for r in _subset(oracle):
        E, ss, st = results[("distinct", "dual", r.sequence)]
        assert st == 0 and (ss, E) == probe_oracle.mfe(r.sequence), r.name
        Eh, E1, sth, st1 = results[("distinct", "pf_helper", _framed(r))]
        assert (sth, st1) == (0, 0) and np.float64(Eh).tobytes() == np.float64(E1).tobytes(), r.name      # bit for bit
        assert abs(Eh - probe_oracle.pf(_framed(r))) < EPF_TOL, r.name


@pytest.mark.parametrize("blocked", [False, True])
def test_two_strip_kernels(results, probe_oracle, blocked):
    """mfe_strip / pf_strip with two strips of 100 nt: plain, and with the blocked multiloop splits (fark) and the second
    tile-product window"""
    for s, t in _strip_cases():
        E, ss, Ep, st, stp = results[("distinct", "strip", s, blocked)]
        assert (st, stp) == (0, 0)
        assert (ss, E) == probe_oracle.mfe(s), s
        assert abs(Ep - probe_oracle.pf(s)) < EPF_TOL, s


def _check_kbest(orc, s, K, E, ss, cut=0):
    """K strings in ascending energy, all different, each with the energy reported for it; the first two energies are the two
    lowest of the structure set"""
    flat = s.replace("&", "")
    live = [(x, e) for x, e in zip(ss, E) if e < INF_REF]
    assert len({x for x, _ in live}) == len(live) and list(E) == sorted(E), (s, E)
    for x, e in live:
        assert orc.eval_structure(flat, x.replace("&", ""), cut) == e, (s, x)
    return live


def test_second_best_and_ranked_structures(results, oracle, probe_oracle):
    """subopt (general), subopt_lds, kbest K = 4 (kbest_kernel) and K = 8 (the shared fill of the ranked lists)"""
    for r in _subset(oracle):
        s = r.sequence
        two = probe_oracle.two_best(s)
        for key in (("distinct", "subopt", s), ("distinct", "second_best", s, True)):
            E2, E12, st = results[key]
            assert st == 0 and E12 == two and E2 == probe_oracle.subopt_energy(s), (r.name, key[1])
    for k, r in enumerate(_subset(oracle)):
        s, two = r.sequence, probe_oracle.two_best(r.sequence)
        for kind, K in ((("kbest_gen", 4),) if k % 2 else (("kbest", 8),)):
            E, ss, st = results[("distinct", kind, s, K)]
            assert st == 0, r.name
            live = _check_kbest(probe_oracle, s, K, E, ss)
            assert tuple((E + [INF_REF])[:2]) == two, (r.name, K)
            if len(s) <= 12:                                               # short enough to rank every structure
                en = sorted(probe_oracle.eval_structure(s, x) for x in _all_structures(s))
                assert list(E) == (en + [INF_REF] * K)[:K], r.name
            assert len(live) == K or len(s) <= 12, r.name


def test_outside_and_edef_lds(results, oracle, probe_oracle):
    """general pf + outside kernels (defect and bpp to 1e-12, as tests/test_kernels_emulated.py) against the record's target and
    the open chain; the fused LDS kernel to EDEF_TOL"""
    for r in _subset(oracle):
        s = r.sequence
        for t in (r.target, "." * len(s)):
            ed, B, st = results[("distinct", "outside", s, t)]
            oe, ob = probe_oracle.ensemble_defect(s, t, want_bpp=True)
            assert st == 0 and abs(ed - oe) < 1e-12 and np.abs(B - ob).max() < 1e-12, (r.name, t)
        ed, bpp, F4, st = results[("distinct", "edef_lds", s, r.target)]
        oe, ob = probe_oracle.ensemble_defect(s, r.target, want_bpp=True)
        assert st == 0 and abs(ed - oe) < EDEF_TOL and np.abs(bpp - ob).max() < EDEF_TOL, r.name


def test_ragged_aux_kernels(results, oracle, probe_oracle):
    seqs, tgts = _ragged_set(oracle)
    assert len({len(s) for s in seqs}) == 4
    for kind in RAGGED_KINDS:
        out = results[("distinct", "ragged", seqs, kind, tgts if kind.startswith("edef") else None)]
        assert out["status"] == [0] * 4, kind
        for k, (s, t) in enumerate(zip(seqs, tgts)):
            if kind.startswith("edef"):
                assert abs(out["edef"][k] - probe_oracle.ensemble_defect(s, t)) < (EDEF_TOL if kind == "edef_lds" else 1e-12), (kind, s)
            else:
                assert tuple(out["E12"][k]) == probe_oracle.two_best(s) and out["E2"][k] == probe_oracle.subopt_energy(s), (kind, s)


# ---- two strands

def test_cofold_kernels(results, probe_oracle):
    """general and LDS co-fold kernels: MFE, the four free energies, E(target) with the nick"""
    for s, t in [(r.sequence, r.target) for r in _co_records()] + [(s, None) for s in _short_pairs()]:
        cut = s.index("&")
        t = t or "." * cut + "&" + "." * (len(s) - cut - 1)
        oss, oe = probe_oracle.cofold_mfe(s)
        f4 = np.array(probe_oracle.cofold_pf(s))
        E, ss, F4, st, Ed = results[("distinct", "co_gen", s, t)]
        assert not any(st) and (ss, E) == (oss, oe), s
        assert np.abs(np.array(F4) - f4).max() < EPF_TOL, s
        assert Ed == probe_oracle.eval_structure(s, t, cut=cut), s
        E, ss, F4, st = results[("distinct", "co_lds", s)]
        assert not any(st) and (ss, E) == (oss, oe), s
        assert np.abs(np.array(F4) - f4).max() < EPF_TOL, s


def test_cofold_second_best_and_ranked_structures(results, probe_oracle):
    """the oracle has no two-strand two_best: short pairs against the enumeration of every co-fold structure, the constructed
    pairs through properties (the lowest energy is the co-fold MFE, the ranked strings evaluate to their energies, the general
    and the LDS kernel agree)"""
    for s in _short_pairs():
        cut, flat = s.index("&"), s.replace("&", "")
        en = sorted(probe_oracle.eval_structure(flat, db, cut) for db in cofold_structures(flat, cut))
        assert en[0] == probe_oracle.cofold_mfe(s)[1], s
        want = tuple((en + [INF_REF])[:2])
        for key in (("distinct", "co_second_best", s), ("distinct", "second_best", s, True)):
            E2, E12, st = results[key]
            assert st == 0 and E12 == want, (s, key[1])
        E, ss, st = results[("distinct", "kbest", s, 8)]
        assert st == 0 and list(E) == (en + [INF_REF] * 8)[:8], s
        _check_kbest(probe_oracle, s, 8, E, ss, cut)
    for r in _co_records():
        s = r.sequence
        cut = s.index("&")
        gen, lds = results[("distinct", "co_second_best", s)], results[("distinct", "second_best", s, True)]
        assert gen == lds and gen[2] == 0 and gen[1][0] == probe_oracle.cofold_mfe(s)[1], r.name
        K = 4 if len(s) % 2 else 8
        E, ss, st = results[("distinct", "kbest", s, K)]
        assert st == 0 and len(_check_kbest(probe_oracle, s, K, E, ss, cut)) == K, r.name
        assert tuple(E[:2]) == gen[1], (r.name, K)


def test_cofold_outside_and_edef_lds(results, probe_oracle):
    """two-strand defect and pair probabilities: the fused LDS kernel equals the general pair of kernels bit for bit (as
    tests/test_edef_lds_emulated.py); FAB is the oracle's; the defect is the definition on the kernel's own matrix; short pairs
    against enumeration under the entry rule of tests/test_cofold_edef_emulated.py (|dP|, |dEdef| < 1e-5 where the integer
    evaluation and the partition function's loop model agree to 1e-6 kcal/mol)"""
    short = _short_pairs()
    for s, t in [(r.sequence, r.target) for r in _co_records()] + [(s, None) for s in short]:
        cut = s.index("&")
        t = t or "." * cut + "&" + "." * (len(s) - cut - 1)
        ed, bpp, F4, st = results[("distinct", "co_outside", s, t)]
        ed2, bpp2, F42, st2 = results[("distinct", "edef_lds", s, t)]
        assert (st, st2) == (0, 0) and ed == ed2 and (bpp == bpp2).all() and F4 == F42, s
        assert abs(F4[3] - probe_oracle.cofold_pf(s)[3]) < EPF_TOL, s
        assert abs(ed - defect_from_matrix(bpp, t)) < 1e-12, s
        if s in short:
            P, F, _ = enumerate_ensemble(probe_oracle, s)
            if abs(F - probe_oracle.cofold_pf(s)[3]) < 1e-6:
                assert np.abs(bpp - P).max() < 1e-5 and abs(ed - defect_from_matrix(P, t)) < 1e-5, s


def test_cofold_pair_probabilities_against_enumeration(results):
    """Under "distinct_sharp" the integer evaluation and the partition function's loop model give every structure the same
    energy (tests/probe_params.py), so the enumeration of every co-fold structure weighted by exp(-E / kT) is a reference for
    the two-strand pair probabilities and the defect of EVERY pair, to EDEF_TOL: rounding is all that separates the two.  Half
    of the pairs at least must have a pair of probability above 0.1 (by the enumeration), so that the matrices are not all
    noise."""
    orc = pyoracle.Oracle(PP.probe_blob("distinct_sharp"))
    pairs = _sharp_pairs()
    checked = informative = 0
    for s, t in pairs:
        ed, bpp, F4, st = results[("distinct_sharp", "co_outside", s, t)]
        ed2, bpp2, F42, st2 = results[("distinct_sharp", "edef_lds", s, t)]
        assert (st, st2) == (0, 0) and ed == ed2 and (bpp == bpp2).all() and F4 == F42, s
        P, F, dbs = enumerate_ensemble(orc, s)
        assert abs(F4[3] - F) < EPF_TOL and abs(F4[3] - orc.cofold_pf(s)[3]) < EPF_TOL, s
        assert np.abs(bpp - P).max() < EDEF_TOL, (s, float(np.abs(bpp - P).max()))
        assert abs(ed - defect_from_matrix(P, t)) < EDEF_TOL, (s, t)
        checked += 1
        informative += P.max() > 0.1 and len(dbs) >= 20
    assert checked == len(pairs) == 10 and informative >= 5, (checked, informative)


def test_self_dimer_kernels(results, probe_oracle):
    for r in LC._selfdimer_records():
        (F_lds, st_lds), (F_ws, st_ws) = results[("distinct", "sd", r.sequence)]
        assert (st_lds, st_ws) == (0, 0) and F_lds == F_ws, r.name
        o = probe_oracle.cofold_pf(r.sequence + "&" + r.sequence)
        assert max(abs(F_lds[c] - o[c]) for c in (0, 2, 3)) < EPF_TOL, r.name


# ---- the special-loop tables at their capacity

def test_full_special_tables(results, full_oracle):
    """64 entries per list: hairpins that hit the first and the last entry of each, and the plain hairpin records, through the
    general, LDS and eval kernels"""
    recs = _full_special_records()
    assert len(recs) == 7 + 6
    got = results[("full_special", "eval", tuple((r.sequence, r.target) for r in recs))]
    for r, e in zip(recs, got):
        assert e == full_oracle.eval_structure(r.sequence, r.target), r.name
        for kind in ("gen", "lds"):
            E, ss, Ep, st, stp = results[("full_special", kind, r.sequence)]
            assert (st, stp) == (0, 0), r.name
            assert (ss, E) == full_oracle.mfe(r.sequence), (kind, r.name)
            assert abs(Ep - full_oracle.pf(r.sequence)) < EPF_TOL, (kind, r.name)
