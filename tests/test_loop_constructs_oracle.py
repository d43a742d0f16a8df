"""The census of tests/constructs.py: the oracle folds every constructed sequence into the loop it was built for (or, beyond
MAXLOOP = 30, refuses to).  The GPU and emulator comparisons of the same records only mean something while this holds: a
record whose intended loop is not in the minimum-free-energy structure tests nothing about that loop.  The counts below are
conditions, not measurements."""
import pytest

from tests import constructs as C


def _size(rec):
    return sum(C.shape_of(rec))


def _interior_census(rows, evaluate):
    """rows: (record, sequence, target, mfe structure, mfe energy), the sequence and target as folded (padded or not).
    -> (in, out): records of size <= 30 folded exactly into their target, larger ones folded into something else whose energy
    is ABOVE that of the target (so the size limit, not the energy model, decides)"""
    n_in = n_out = 0
    for r, seq, tgt, ss, e in rows:
        assert e == evaluate(seq, ss), r.name
        if _size(r) <= C.MAXLOOP:
            assert ss == tgt, r.name
            n_in += 1
        else:
            assert ss != tgt and not C.has_loop(ss, r, tgt.replace("&", "").index("(")), r.name
            assert evaluate(seq, tgt) < e, r.name
            n_out += 1
    return n_in, n_out


def test_interior_every_shape_up_to_35(oracle):
    recs = C.interior()
    assert len(recs) == 666 and len({r.sequence for r in recs}) == 666
    assert all(len(r.sequence) == len(r.target) == 20 + _size(r) and C.has_loop(r.target, r) for r in recs)
    fold = [oracle.mfe(r.sequence) for r in recs]
    rows = [(r, r.sequence, r.target) + f for r, f in zip(recs, fold)]
    assert _interior_census(rows, oracle.eval_structure) == (496, 170)
    e = {r.name: f[1] for r, f in zip(recs, fold)}
    assert (e["int_15x15"], e["int_0x30"], e["int_1x29"], e["int_2x28"], e["int_13x17"]) == (-1421, -1181, -1121, -1121, -1221)
    # above the limit the inner hairpin alone is left (the two bulges of size 31 keep one more or one fewer stacked pair)
    assert {f[1] for r, f in zip(recs, fold) if _size(r) > 30} == {-1070, -1050, -980}
    assert (e["int_0x31"], e["int_31x0"]) == (-1050, -980)
    th = C.thinned_interior()
    assert {r.name for r in th} <= {r.name for r in recs} and len(th) == 260
    assert sum(_size(r) in (30, 31) for r in th) == 31 + 32


@pytest.mark.parametrize("L", [72, 100, 230])
def test_interior_padded_frames(oracle, L):
    """poly-A around the construct changes nothing, wherever it sits; the offsets cover both ends of the frame and (nearly)
    every residue of the tower, ring and tower-block periods"""
    recs = C.interior()
    offs = set()
    for k in C.OFFSET_RULES:
        padded = [C.pad(r, L, k) for r in recs]
        offs |= {p[2] for p in padded}
        _, Emfe, ss, Ed = oracle.score_batch([p[0] for p in padded], ["." * L])
        rows = [(r, p[0], p[1], s, int(e)) for r, p, s, e in zip(recs, padded, ss, Emfe)]
        assert _interior_census(rows, oracle.eval_structure) == (496, 170), (L, k)
    assert 0 in offs
    assert any(C.pad(r, L, k)[2] == L - len(r.sequence) for r in recs for k in C.OFFSET_RULES)      # flush right
    for m in (28, 32, 64):
        want = min(m, L - 55 + 1)                # every residue that the longest record's room allows
        assert len({o % m for o in offs}) >= want, (L, m)


def test_cofold_every_shape_and_the_nicked_loops(oracle):
    for common in (False, True):
        recs = C.cofold(common=common)
        assert len(recs) == 666
        if common:
            assert {len(r.sequence) for r in recs} == {54} and len({(C.cut_of(r), len(r.sequence)) for r in recs}) == 36
        fold = [oracle.cofold_mfe(r.sequence) for r in recs]
        rows = [(r, r.sequence, r.target) + f for r, f in zip(recs, fold)]
        cut = {r.sequence: C.cut_of(r) for r in recs}
        assert _interior_census(rows, lambda seq, ss: oracle.eval_structure(seq, ss, cut=cut[seq])) == (496, 170)
    # the nick inside the u1 run: an exterior loop, no size limit -- both helices form at every size
    recs = C.nicked()
    assert {_size(r) for r in recs} == set(C.NICKED_SIZES)
    for r in recs:
        ss, e = oracle.cofold_mfe(r.sequence)
        assert ss == r.target and e == oracle.eval_structure(r.sequence, ss, cut=C.cut_of(r)), r.name


def test_hairpins_and_special_loops(oracle):
    recs = C.hairpin()
    assert len(recs) == 68 + 30 and len(C.special_hairpins()) == 30
    for r in recs:
        ss, e = oracle.mfe(r.sequence)
        assert ss == r.target and C.has_loop(ss, r), r.name
        assert e == oracle.eval_structure(r.sequence, ss), r.name


def test_multiloops(oracle):
    recs = C.multiloop()
    assert len(recs) == 10 and max(len(r.sequence) for r in recs) == 96
    for r in recs:
        ss, e = oracle.mfe(r.sequence)
        assert ss == r.target and C.has_loop(ss, r), r.name
        assert e == oracle.eval_structure(r.sequence, ss), r.name
    loose = C.multiloop(pinned=False)
    assert [r.name for r in loose if oracle.mfe(r.sequence)[0] != r.target] == ["ml_k3_a0", "ml_k5_a0", "ml_k6_a0"]


def test_small_loops_all_closing_pairs(oracle):
    """the plain recipe (every candidate filling) reaches the intended loop in 29 ... 62 % of a shape's records and in 35 or 36
    of the 36 closing-pair combinations (none of the four 0 x 1 fillings between UG and GU does, nor any sampled 1 x 5 one of
    one combination); rejection sampling with the oracle keeps every candidate that does, plus one record of a combination
    without any: at least 95 % then.  Every base occurs at every loop position of every shape among the kept records."""
    raw = C.small()
    assert len(raw) == 2 * 144 + 10 * 576
    picked = C.small(oracle)
    assert {r.name for r in picked} <= {r.name for r in raw}
    combo = lambda r: tuple(r.name.split("_")[2:4])
    for recs, floor in ((raw, 0.25), (picked, 0.95)):
        for shape in C.SMALL_SHAPES:
            fam = [r for r in recs if C.shape_of(r) == shape]
            hit = [r for r in fam if C.has_loop(oracle.mfe(r.sequence)[0], r)]
            assert len(hit) >= floor * len(fam), (shape, len(hit), len(fam))
            assert len({combo(r) for r in hit}) >= (35 if shape in ((0, 1), (1, 5)) else 36), shape
            for r in hit:
                ss, e = oracle.mfe(r.sequence)
                assert e == oracle.eval_structure(r.sequence, ss), r.name
            if recs is picked:
                i, j, p, q = hit[0].intended_loop
                for pos in list(range(i + 1, p)) + list(range(q + 1, j)):
                    assert {r.sequence[pos] for r in hit} == set("ACGU"), (shape, pos)
    assert sum(1 for r in picked if C.has_loop(oracle.mfe(r.sequence)[0], r)) == len(picked) - 2


def test_selfdimer_loops_straddle_the_limit(oracle):
    for tail, lens in ((0, (12, 46)), (20, (32, 66))):
        recs = C.selfdimer(tail)
        assert (len(recs[0].sequence), len(recs[-1].sequence)) == lens and len(recs) == 18
        for u, r in enumerate(recs):
            s = r.sequence
            n = len(s) - tail
            ss, e = oracle.cofold_mfe(s + "&" + s)
            a, b = ss.split("&")
            full = "((((" + "." * u + "((((" + "." * u + "((((" + "." * tail
            if 2 * u <= C.MAXLOOP:
                assert a == full and b[:n] == full[:n].replace("(", ")")[::-1], r.name      # three helices, two u x u loops
            else:
                assert a != full, r.name
