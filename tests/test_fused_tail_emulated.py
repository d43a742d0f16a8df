"""CPU emulation (tests/emu) of the two roles pairs of the fused launch on constructed records (tests/constructs.py): the
two-workgroup MFE fold, whose traceback scans the interior candidates by groups of rounds and takes its sectors from a queue
of LDS atomics, and the partition function's main and helper workgroups.
Structures, energies and the bits of Epf must be those of the one-workgroup emulated kernels (and the oracle's).

The records put the interior hit into scan rounds 0, 1, 2, 5 and 7 (candidate index = canonical order, 64 per round), into every
table-driven kind, into the tetraloop table (the other special-hairpin tables: the "full_special" probe parameters) and into
multiloops of two and three branches."""
import numpy as np
import pytest

from tests import constructs as C
from tests.emu.emu import Emu

L_FRAME = 60
SHAPES = ((0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (0, 7), (2, 5), (5, 4), (13, 17), (25, 5))


@pytest.fixture(scope="module")
def emu(blob):
    return Emu(blob)


def _round_of(u1, u2):
    """scan round of candidate (u1, u2): its index in the canonical order (u1 ascending, u2 ascending) over 64"""
    return (sum(C.MAXLOOP + 1 - u for u in range(u1)) + u2) // 64


@pytest.fixture(scope="module")
def frames():
    assert sorted({_round_of(*s) for s in SHAPES}) == [0, 1, 2, 5, 7]
    hp = {r.name: r for r in C.hairpin()}
    special = [r for r in C.hairpin() if r.name.startswith("hp_special_")]      # (Turner-1999: tetraloops; the other tables below)
    ml = {r.name: r for r in C.multiloop()}
    recs = [C.interior_record(*s) for s in SHAPES] + [special[0], special[-1], hp["hp_3"], hp["hp_30"], ml["ml_k2_a1"], ml["ml_k3_a2"]]
    return [(r,) + C.pad(r, L_FRAME, 11) for r in recs]


def test_two_workgroup_mfe_matches_one_workgroup(emu, oracle, frames):
    seqs = [f[1] for f in frames]
    E2, ss2, st2 = emu.mfe_dual(seqs, nt=256)
    E1, ss1, st1 = emu.mfe(seqs, nt=-256)
    assert not st2.any() and not st1.any()
    assert ss2 == ss1 and (E2 == E1).all()
    hits = 0
    for (r, s, t, off), ss, e in zip(frames, ss2, E2):
        assert (ss, int(e)) == oracle.mfe(s), r.name
        hits += C.has_loop(ss, r, off)
    assert hits >= len(frames) - 2, hits                     # the records fold into the loop they were built for


def test_special_hairpin_tables_full():
    """Turner-1999 has tetraloops only; the "full_special" probe (tests/probe_params.py) fills the tri-, tetra- and hexaloop
    tables to their capacity of one entry per lane.  A hairpin closed by an entry of each table, first, middle and last in table
    order, through the two-workgroup fold's traceback."""
    from oracle import pyoracle
    from tests import probe_params as PP
    blob = PP.probe_blob("full_special")
    e, orc = Emu(blob), pyoracle.Oracle(blob)
    seqs = []
    for table in PP.special_loops("full_special"):
        assert len(table) == PP.MAX_SPECIAL
        for loop, _ in (table[0], table[len(table) // 2], table[-1]):
            s, t = PP.special_hairpin(loop)
            seqs.append(("A" * 11 + s + "A" * L_FRAME)[:L_FRAME])
    E2, ss2, st2 = e.mfe_dual(seqs, nt=256)
    E1, ss1, st1 = e.mfe(seqs, nt=-256)
    assert not st2.any() and not st1.any()
    assert ss2 == ss1 and (E2 == E1).all()
    for s, ss, en in zip(seqs, ss2, E2):
        assert (ss, int(en)) == orc.mfe(s), s


def test_pf_main_and_helper_match_one_workgroup(emu, oracle, frames):
    seqs = [f[1] for f in frames]
    Eh, sth = emu.pf(seqs, nt=-257)
    E1, st1 = emu.pf(seqs, nt=-256)
    assert not sth.any() and not st1.any()
    assert (Eh.view(np.int64) == E1.view(np.int64)).all()
    for k, s in enumerate(seqs):
        assert abs(Eh[k] - oracle.pf(s)) < 1e-9, frames[k][0].name
