"""Loop-model edge cases on every fold path of the GPU build: the constructed sequences of tests/constructs.py (every interior
loop shape up to 35 bases, the small-loop tables over all closing pairs, long and special hairpins, multiloops, the two-strand
and self-dimer forms) against the oracle on the same sequence.  Random sequences never fold into a 13 x 17 or a 0 x 30 loop;
these do, and tests/test_loop_constructs_oracle.py keeps that true.  MFE strings, Emfe and E(target) are bit-exact, Epf to
EPF_TOL_ORACLE; every row of the score_batch path matrix asserts the path it took (last_fused, last_workgroups).  The engine
exposes no such indicator for the ragged call and the auxiliary entry points: there the "*_lds" option selects the kernel and the
test can only read the option back.  Each row prints its census: records compared and how many of them hold the intended
loop in their MFE structure."""
import numpy as np
import pytest

from tests import constructs as C
from tests.test_gpu_parity import EDEF_TOL, EPF_TOL_ORACLE
from tests.test_self_dimer_gpu import F4_TOL

pytestmark = pytest.mark.gpu

MFE_FARK_MIN_STRIPS = 4         # the one option used here that cannot be read back: blocked MFE splits from four strips on
SWEEP_SHAPES = ((15, 15), (0, 30), (1, 29), (2, 28), (15, 16))
INF_REF = 10000000


@pytest.fixture(scope="module")
def eng():
    from desirna_amd import engine
    e = engine.Engine(max_R=128, max_L=400, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fam(oracle):
    """the record sets, built once.  small: every oracle-checked filling (up to 16) of every closing-pair combination, at
    every frame length.  Each row of the matrix runs in two parts, "shapes" (interior, thinned on the long frames, + hairpin +
    multiloop) and "small"."""
    ml = C.multiloop() + C.multiloop(pinned=False)
    d = {"interior": C.interior(), "thin": C.thinned_interior(), "small": C.small(oracle, keep=16), "hairpin": C.hairpin(),
         "multiloop": ml}
    d["short", "shapes"] = d["interior"] + d["hairpin"] + d["multiloop"]
    d["long", "shapes"] = d["thin"] + d["hairpin"] + d["multiloop"]
    d["short", "small"] = d["long", "small"] = d["small"]
    return d


PARTS = pytest.mark.parametrize("part", ["shapes", "small"])


class _options:
    """engine options for the length of a with-block; what they were on entry comes back whatever happens inside"""

    def __init__(self, eng, **opts):
        self.eng, self.opts = eng, opts
        self.saved = {}

    def __enter__(self):
        try:
            for n, v in self.opts.items():
                self.saved[n] = MFE_FARK_MIN_STRIPS if n == "mfe_fark_min_strips" else self.eng.get_option(n)
                self.eng.set_option(n, v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            self.eng.set_option(n, v)


_REF = {}


def _reference(oracle, frames):
    """oracle answers for (record, sequence, target, offset) frames of one length, in chunks of 128 sequences: Epf, Emfe, MFE
    strings and E(every target of the chunk).  Computed once per set of frames and shared by the rows that use it."""
    key = hash(tuple(f[1] for f in frames))
    if key not in _REF:
        chunks = []
        for b in range(0, len(frames), 128):
            fr = frames[b:b + 128]
            Epf, Emfe, ss, Ed = oracle.score_batch([f[1] for f in fr], [f[2] for f in fr])
            chunks.append((fr, Epf, Emfe, ss, Ed))
        _REF[key] = chunks
    return _REF[key]


def _frames(recs, L, k):
    out = []
    for r in recs:
        if len(r.sequence) <= L:
            s, t, o = C.pad(r, L, k)
            out.append((r, s, t, o))
    return out


def _census(label, rows):
    """rows: (record, offset, GPU structure).  Prints records / records with the intended loop per family, returns the same."""
    out = {}
    for r, o, ss in rows:
        n, h = out.get(r.family, (0, 0))
        out[r.family] = (n + 1, h + bool(C.has_loop(ss, r, o)))
    print("CENSUS %-34s %s" % (label, "  ".join("%s %d/%d" % (f, h, n) for f, (n, h) in sorted(out.items()))))
    return out


def _row(eng, oracle, frames, label, opts=None, per_call=128, wgs_per_seq=None, fused=None, mfe_only=False, pk=False):
    """one row of the path matrix: the frames through score_batch under `opts`, per_call sequences at a time, against the oracle"""
    from desirna_amd import engine as E
    flags = E.NEED_MFE if mfe_only else E.NEED_PF | E.NEED_MFE | E.NEED_EVAL
    if pk:
        flags |= E.NEED_PK
    rows = []
    with _options(eng, **(opts or {})):
        for fr, Epf, Emfe, ss, Ed in _reference(oracle, frames):
            for b in range(0, len(fr), per_call):
                sub = fr[b:b + per_call]
                R = len(sub)
                seqs = [f[1] for f in sub]
                eng.set_targets([f[2] for f in sub])
                out = eng.score_batch(seqs, flags)
                if fused is not None:
                    assert eng.get_option("last_fused") == fused, label
                if wgs_per_seq is not None:
                    assert eng.get_option("last_workgroups") == wgs_per_seq * R, (label, eng.get_option("last_workgroups"), R)
                for k, f in enumerate(sub):
                    want = oracle.pk_struct(f[1], ss[b + k]) if pk else ss[b + k]
                    assert out["mfe_ss"][k] == want, (label, f[0].name, f[3], out["mfe_ss"][k], want)
                    assert int(out["Emfe"][k]) == int(Emfe[b + k]), (label, f[0].name, f[3])
                    rows.append((f[0], f[3], out["mfe_ss"][k].replace("[", ".").replace("]", ".")))
                if not mfe_only:
                    d = np.abs(out["Epf"] - Epf[b:b + R])
                    assert d.max() < EPF_TOL_ORACLE, (label, sub[int(d.argmax())][0].name, float(d.max()))
                    bad = np.argwhere(out["Ed"] != Ed[b:b + R, b:b + R])
                    assert not len(bad), (label, sub[bad[0][0]][0].name, "target of", sub[bad[0][1]][0].name)
    return _census(label, rows)


def _check(census, part, n, hits):
    """shapes: the loop in the MFE of every interior shape up to 30 and of none above; small: at least 95 % with the loop"""
    if part == "shapes":
        assert census["interior"] == (n, hits), census
    else:
        assert census["small"][1] >= 0.95 * census["small"][0] and census["small"][0] >= 2400, census


# ---- the path matrix: interior + small + hairpin + multiloop

@PARTS
def test_lds_kernels_72(eng, oracle, fam, part):
    """defaults at 72 nt: mfe_lds_kernel and pf_lds_kernel, one workgroup per fold, no helper (what does not fit 72 nt is left
    to the rows below: hairpins of 63 bases and more, multiloops of five and six branches)"""
    fr = _frames(fam["short", part], 72, 0)
    left_out = {r.name for r in fam["short", part]} - {f[0].name for f in fr}
    assert left_out == ({"hp_%d" % h for h in range(63, 71)} | {"ml_k5_a1", "ml_k6_a1", "ml_k5_a2", "ml_k6_a2", "ml_k6_a0"} if part == "shapes" else set())
    _check(_row(eng, oracle, fr, "L72 defaults " + part, wgs_per_seq=2, fused=0), part, 666, 496)


@PARTS
def test_lds_kernels_100(eng, oracle, fam, part):
    fr = _frames(fam["short", part], 100, 0)
    _check(_row(eng, oracle, fr, "L100 dual=0 pf_helper=0 " + part, {"dual": 0, "pf_helper": 0}, wgs_per_seq=2, fused=0), part, 666, 496)


@PARTS
def test_two_workgroup_folds_100(eng, oracle, fam, part):
    """mfe_dual_kernel and the partition function with its helper workgroup (E(targets) evaluated by the helpers), two launches"""
    fr = _frames(fam["short", part], 100, 11)
    c = _row(eng, oracle, fr, "L100 dual=2 pf_helper=1 fused=0 " + part, {"dual": 2, "pf_helper": 1, "fused": 0}, per_call=32, wgs_per_seq=4, fused=0)
    _check(c, part, 666, 496)


@PARTS
def test_fused_launch_100(eng, oracle, fam, part):
    fr = _frames(fam["short", part], 100, -1)
    c = _row(eng, oracle, fr, "L100 dual=2 pf_helper=1 fused=1 " + part, {"dual": 2, "pf_helper": 1, "fused": 1}, per_call=32, wgs_per_seq=4, fused=1)
    _check(c, part, 666, 496)


@PARTS
def test_two_strips_100(eng, oracle, fam, part):
    fr = _frames(fam["short", part], 100, 0)
    _check(_row(eng, oracle, fr, "L100 strips=2 " + part, {"strips": 2}, wgs_per_seq=4, fused=0), part, 666, 496)


@PARTS
def test_strip_kernels_230(eng, oracle, fam, part):
    """two strips per fold, plain multiloop splits; and the same strips with the blocked splits (MFE only)"""
    fr = _frames(fam["long", part], 230, 11)
    _check(_row(eng, oracle, fr, "L230 defaults " + part, wgs_per_seq=4, fused=0), part, 260, 186)
    c = _row(eng, oracle, fr, "L230 mfe_fark_min_strips=2 " + part, {"mfe_fark_min_strips": 2}, wgs_per_seq=2, mfe_only=True)
    _check(c, part, 260, 186)


@PARTS
def test_general_kernels_230(eng, oracle, fam, part):
    fr = _frames(fam["long", part], 230, 11)
    _check(_row(eng, oracle, fr, "L230 strips=0 " + part, {"strips": 0}, wgs_per_seq=2, fused=0), part, 260, 186)


@PARTS
def test_strip_kernels_400(eng, oracle, fam, part):
    """four strips per fold: the blocked MFE splits are the default from four strips on, so "mfe_fark_min_strips" = 2 is the
    default path again and = 5 the plain form (both MFE only)"""
    fr = _frames(fam["long", part], 400, -1)
    _check(_row(eng, oracle, fr, "L400 defaults " + part, wgs_per_seq=8, fused=0), part, 260, 186)
    _row(eng, oracle, fr, "L400 mfe_fark_min_strips=2 " + part, {"mfe_fark_min_strips": 2}, wgs_per_seq=4, mfe_only=True)
    _row(eng, oracle, fr, "L400 mfe_fark_min_strips=5 " + part, {"mfe_fark_min_strips": 5}, wgs_per_seq=4, mfe_only=True)


def _sweep(L):
    out = []
    for u1, u2 in SWEEP_SHAPES:
        r = C.interior_record(u1, u2)
        room = L - len(r.sequence)
        for off in sorted(set(range(0, room + 1, 7)) | {room}):
            s, t, o = C.pad(r, L, offset=off)
            out.append((r, s, t, o))
    return out


def test_offset_sweep_across_strip_boundaries(eng, oracle):
    """15 x 15, 0 x 30, 1 x 29, 2 x 28 and 15 x 16 at every seventh offset and flush right: the outer pair, the inner pair and
    the 32-diagonal look-back each straddle every strip boundary (column 115 at 230 nt; 100, 200, 300 at 400 nt)"""
    for L, wgs, opts in ((230, 4, {}), (400, 8, {"mfe_fark_min_strips": 2})):
        fr = _sweep(L)
        S = wgs // 2
        for s in range(1, S):
            for b in range(L * s // S - 3, L * s // S + 4):            # whichever column near L s / S the strips part at
                for lo, hi in ((0, 2), (2, 3), (3, 1)):                # ... lies in the 5' side of the loop, under the inner pair, in the 3' side
                    assert any(f[3] + f[0].intended_loop[lo] < b <= f[3] + f[0].intended_loop[hi] for f in fr), (L, b, lo)
        c = _row(eng, oracle, fr, "L%d offset sweep" % L, opts, wgs_per_seq=wgs, fused=0)
        assert c["interior"] == (len(fr), sum(1 for f in fr if C.shape_of(f[0]) != (15, 16)))


def test_ragged_every_interior_record_in_one_launch(oracle, fam):
    """all 666 records at their native lengths (20 ... 55 nt) in ONE score_ragged call (an engine of its own: the call takes
    max_R sequences at most).  The ragged call writes no last_workgroups / last_fused; that the batch is not cut into chunks
    shows in workspace_slots, and that no fold lost a partner in sync_fallbacks."""
    from desirna_amd import engine as E
    recs = fam["interior"]
    big = E.Engine(max_R=len(recs), max_L=55, device=0)
    try:
        assert big.get_option("workspace_slots") >= len(recs)
        big.set_targets_ragged([r.target for r in recs])
        out = big.score_ragged([r.sequence for r in recs], list(range(len(recs))))
        assert big.get_option("sync_fallbacks") == 0
    finally:
        big.close()
    rows = []
    for k, r in enumerate(recs):
        ss, e = oracle.mfe(r.sequence)
        assert (out["mfe_ss"][k], int(out["Emfe"][k])) == (ss, e), r.name
        assert abs(float(out["Epf"][k]) - oracle.pf(r.sequence)) < EPF_TOL_ORACLE, r.name
        assert int(out["Ed"][k]) == oracle.eval_structure(r.sequence, r.target), r.name
        rows.append((r, 0, out["mfe_ss"][k]))
    assert _census("ragged native lengths", rows)["interior"] == (666, 496)


def test_pseudoknot_rounds_at_the_size_limit(eng, oracle, fam):
    """NEED_PK on the 126 records of sizes 29 ... 32 at 100 nt: the re-folds run the same fill on masked sequences"""
    recs = [r for r in fam["interior"] if 29 <= sum(C.shape_of(r)) <= 32]
    assert len(recs) == 126
    # (63 per call: room for the partition function's helpers beside the one-workgroup MFE folds -- three workgroups per sequence)
    c = _row(eng, oracle, _frames(recs, 100, 11), "L100 NEED_PK sizes 29-32", per_call=63, wgs_per_seq=3, fused=0, pk=True)
    assert c["interior"] == (126, 61)


# ---- the other entry points

def test_ensemble_defect(eng, oracle, fam):
    """inside + outside recursion against each record's own target: interior at 60 nt, hairpins at 80 nt"""
    n = 0
    for recs, L in ((fam["interior"], 60), (fam["hairpin"], 80)):
        for r, s, t, o in _frames(recs, L, 0):
            eng.set_targets([t])
            ed, bpp = eng.ensemble_defect([s], want_bpp=True)
            oe, ob = oracle.ensemble_defect(s, t, want_bpp=True)
            assert abs(ed[0] - oe) < EDEF_TOL, (r.name, ed[0], oe)
            assert np.abs(bpp[0] - ob).max() < EDEF_TOL, r.name
            n += 1
    assert n == 666 + 98
    print("CENSUS ensemble_defect records", n)


def _groups(recs, limit):
    """records padded to `limit` (or left at their own length when longer), grouped by length"""
    g = {}
    for r in recs:
        L = max(limit, len(r.sequence))
        g.setdefault(L, []).append((r,) + C.pad(r, L, 0))
    return g


def _two_best_reference(oracle, groups):
    key = ("two_best", hash(tuple(f[1] for L in sorted(groups) for f in groups[L])))
    if key not in _REF:
        _REF[key] = {f[1]: (oracle.two_best(f[1]), oracle.subopt_energy(f[1]), oracle.mfe(f[1])) for L in groups for f in groups[L]}
    return _REF[key]


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("family,limit", [("interior", 60), ("small", 32), ("hairpin", 79)])
def test_second_best_energy(eng, oracle, fam, family, limit, lds):
    """the two lowest energies under both "subopt_lds" settings (the LDS kernel takes up to subopt_lds_max = 79 nt).  For an
    interior record up to size 30 they are (the loop structure, the inner hairpin alone), beyond it the other way round or worse"""
    groups = _groups(fam[family], limit)
    ref = _two_best_reference(oracle, groups)
    with _options(eng, subopt_lds=lds):
        assert eng.get_option("subopt_lds") == lds
        for L, fr in sorted(groups.items()):
            for b in range(0, len(fr), 128):
                sub = fr[b:b + 128]
                E2, E12 = eng.subopt_energy([f[1] for f in sub], want_both=True)
                for k, f in enumerate(sub):
                    two, e2, (mss, me) = ref[f[1]]
                    assert tuple(int(x) for x in E12[k]) == two, (f[0].name, lds)
                    assert int(E2[k]) == e2 and int(E12[k, 0]) == me, (f[0].name, lds)
    if family == "interior":
        assert oracle.two_best(C.interior_record(13, 17).sequence) == (-1221, -1070)       # (unpadded: no dangling A on the helix ends)
        for f in groups[60]:
            two, _, (mss, me) = ref[f[1]]
            if sum(C.shape_of(f[0])) <= C.MAXLOOP:
                assert two[0] == oracle.eval_structure(f[1], f[2]) and two[1] > two[0]
            else:
                assert two[0] > oracle.eval_structure(f[1], f[2])


@pytest.mark.parametrize("family,limit", [("interior", 60), ("small", 32), ("hairpin", 79)])
def test_ranked_structures(eng, oracle, fam, family, limit):
    """K = 4 lowest structures: rank 0 is the MFE structure with its energy, energies ascend, rank 1 is the oracle's second best,
    every string is worth its energy"""
    groups = _groups(fam[family], limit)
    ref = _two_best_reference(oracle, groups)
    for L, fr in sorted(groups.items()):
        for b in range(0, len(fr), 128):
            sub = fr[b:b + 128]
            En, ss = eng.subopt_structs([f[1] for f in sub], 4)
            for k, f in enumerate(sub):
                two, _, (mss, me) = ref[f[1]]
                e = [int(x) for x in En[k]]
                assert e[0] == me and (ss[k][0] == mss or two[0] == two[1]), f[0].name        # (equal energies: the order is the engine's own)
                assert e == sorted(e) and e[1] == two[1], f[0].name
                for x, v in zip(ss[k], e):
                    if v < INF_REF:
                        assert oracle.eval_structure(f[1], x) == v, (f[0].name, x)


def _cofold_calls(fam_co):
    """pairs that share their strand lengths, one call each: the 36 u1 groups of the padded two-strand form, the nicked ones singly"""
    g = {}
    for r in fam_co:
        g.setdefault((C.cut_of(r), len(r.sequence)), []).append(r)
    return [g[k] for k in sorted(g)]


@pytest.mark.parametrize("lds", [1, 0])
def test_cofold_every_shape_and_the_nicked_loops(eng, oracle, lds):
    """co-fold MFE, the four partition-function energies and E(target) with the nick, LDS (54 nt <= cofold_lds_max) and general
    kernels: the interior loop closed across the nick obeys the size limit, the nicked (exterior) loop does not"""
    calls = _cofold_calls(C.cofold(common=True) + C.nicked())
    assert len(calls) == 36 + len(C.nicked())
    rows = []
    with _options(eng, cofold_lds=lds):
        assert eng.get_option("cofold_lds") == lds and eng.get_option("cofold_lds_max") >= 54
        for recs in calls:
            eng.set_targets([r.target.replace("&", "") for r in recs])
            out = eng.cofold_batch([r.sequence for r in recs])
            for k, r in enumerate(recs):
                key = ("co", r.sequence)
                if key not in _REF:
                    _REF[key] = (oracle.cofold_mfe(r.sequence), oracle.cofold_pf(r.sequence),
                                 oracle.eval_structure(r.sequence, r.target, cut=C.cut_of(r)))
                (oss, oe), f4, oed = _REF[key]
                assert (out["mfe_ss"][k], int(out["Emfe"][k])) == (oss, oe), (r.name, lds)
                got = [float(out[x][k]) for x in ("FA", "FB", "FcAB", "FAB")]
                assert max(abs(g - o) for g, o in zip(got, f4)) < EPF_TOL_ORACLE, (r.name, lds)
                assert int(out["Ed"][k, k]) == oed, (r.name, lds)
                rows.append((r, 0, out["mfe_ss"][k].replace("&", "")))
    c = _census("cofold_batch cofold_lds=%d" % lds, rows)
    assert c["cofold"] == (666, 496) and c["nicked"] == (len(C.nicked()),) * 2


def test_cofold_second_best_energy(eng, oracle):
    """both "subopt_lds" settings bit for bit, and E1 is the co-fold MFE"""
    calls = _cofold_calls(C.cofold(common=True) + C.nicked())
    res = []
    for lds in (1, 0):
        with _options(eng, subopt_lds=lds):
            res.append([eng.cofold_subopt_energy([r.sequence for r in recs], want_both=True) for recs in calls])
    for recs, (E2a, E12a), (E2b, E12b) in zip(calls, res[0], res[1]):
        assert E2a.tobytes() == E2b.tobytes() and E12a.tobytes() == E12b.tobytes(), recs[0].name
        for k, r in enumerate(recs):
            assert int(E12a[k, 0]) == oracle.cofold_mfe(r.sequence)[1], r.name
            assert int(E12a[k, 0]) <= int(E12a[k, 1])


@pytest.mark.parametrize("tail", [0, 20])
def test_self_dimer_symmetric_loops(eng, oracle, tail):
    """s & s of GGCC A^u GCGC A^u GGCC: symmetric u x u loops of sizes 0 ... 34; with 20 A appended the lengths cross
    self_dimer_lds_max (62).  Against the oracle and cofold_batch(s & s) as in test_self_dimer_gpu.py, and LDS against workspace
    kernel bit for bit"""
    from desirna_amd import engine as E
    M = eng.get_option("self_dimer_lds_max")
    recs = C.selfdimer(tail)
    if tail:
        assert min(len(r.sequence) for r in recs) <= M < max(len(r.sequence) for r in recs)
    for r in recs:
        s = r.sequence
        out = []
        for lds in (1, 0):
            with _options(eng, self_dimer_lds=lds):
                out.append(eng.self_dimer([s]))
        S = [np.stack([o["FA"], o["FA"], o["FcAA"], o["FAA"]], axis=1) for o in out]
        assert S[0].tobytes() == S[1].tobytes() and out[0]["oligo_fraction"].tobytes() == out[1]["oligo_fraction"].tobytes(), r.name
        co = eng.cofold_batch([s + "&" + s], E.NEED_PF)
        G = np.array([co["FA"][0], co["FB"][0], co["FcAB"][0], co["FAB"][0]])
        assert np.abs(S[0][0] - G).max() < F4_TOL, r.name
        o = oracle.cofold_pf(s + "&" + s)
        assert max(abs(S[0][0, c] - o[c]) for c in (0, 2, 3)) < F4_TOL, r.name
