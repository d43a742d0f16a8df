"""The engine as a stateful object: every entry point after and before every other on ONE engine, after failed calls, and on
workspaces filled with a poison byte (option "poison").  Its entry points share mutable device state -- the PF tables are the
samplers' tables and, read as int32, the second-best fold's; the outside workspace is the MEA table; d_Emfe / d_Epf double as
E2 / E12; one array holds both sets of status words; half the buffers exist or grow depending on what was called before -- and a
fresh allocation usually reads as zeros, so a kernel that reads a cell it never wrote, or a host path that forgets a status word,
passes every test that builds an engine for one feature.

The operations are the table of tests/call_order_ops.py (one engine size, lengths on both sides of every path switch).  Each is
run once on a fresh engine of its own and anchored on the oracle (the baseline); every other result must equal that baseline
BIT FOR BIT, which is what the project promises: Epf bitwise equal however the fold is run, tile products the same bits whoever
computes them, the defect independent of batch composition, the samplers' seed contract.  ``sync_fallbacks`` is not asserted: on
a shared card a lost partner is legitimate and the redo gives the same bits.

Poison bytes are 0xFF (NaN in every double table, -1 in every int32 / int16 table: a stale read changes a sum or a minimum) and
0x00 (the fresh allocation the baseline had); no others -- a pattern that reads as a huge positive count would turn a stale list
length into a wild loop bound, and these tests detect stale reads by their values."""
import pytest

from tests import call_order_ops as ops

pytestmark = pytest.mark.gpu

BAD_CHAR, BAD_ARG = -4, -1                       # DRNA_ERR_SEQUENCE, DRNA_ERR_ARG (include/desirna_amd.h)


_DEVICE_ERROR = []                               # the first HIP / device error of this module: nothing more is started on the GPU after it


def _engine():
    from desirna_amd import engine
    if _DEVICE_ERROR:
        pytest.fail("an earlier case met a device error (%s): no further GPU work in this module" % _DEVICE_ERROR[0])
    return engine.Engine(max_R=ops.MAX_R, max_L=ops.MAX_L, device=0)


def _run(op, e, installed=False, seqs=None):
    """op.run(e) (installed: the call alone, on `seqs` if given); a device error ends the module's GPU work"""
    from desirna_amd import engine
    if _DEVICE_ERROR:
        pytest.fail("an earlier case met a device error (%s): no further GPU work in this module" % _DEVICE_ERROR[0])
    try:
        return op.run_installed(e, seqs) if installed else op.run(e)
    except engine.EngineError as err:
        if err.code == -3:
            _DEVICE_ERROR.append("%s: %s" % (op.name, err))
        raise


@pytest.fixture(scope="module")
def baseline(oracle):
    """every operation once on a fresh engine of its own, anchored on the oracle"""
    out = {}
    for op in ops.OPS:
        e = _engine()
        try:
            out[op.name] = _run(op, e)
        finally:
            e.close()
        op.anchor(oracle, out[op.name])
    return out


@pytest.fixture(scope="module")
def eng():
    """the shared engine: state piles up across the cases of this module"""
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def warm(baseline):
    """an engine on which every operation has run once, so every lazily allocated buffer exists (and holds another call's data)"""
    e = _engine()
    for op in ops.OPS:
        _same(op, _run(op, e), baseline, "warm-up")
    yield e
    e.close()


def _same(op, got, baseline, what):
    field = ops.first_difference(op, got, baseline[op.name])
    assert field is None, "%s: %s differs from the fresh engine's in %r" % (what, op.name, field)


@pytest.mark.parametrize("name", ops.NAMES)
def test_after_and_before(eng, baseline, name):
    """A, B, A, B for every other operation B: A after A's own kind of state, A after B and B after A for every ordered pair"""
    a = ops.BY_NAME[name]
    for b in ops.OPS:
        if b is a:
            continue
        for k in (1, 2):
            _same(a, _run(a, eng), baseline, "%s (run %d) in the chain with %s" % (a.name, k, b.name))
            _same(b, _run(b, eng), baseline, "%s (run %d) after %s" % (b.name, k, a.name))


def _score_ops():
    return ops.BY_NAME["score_L200_R9"], ops.BY_NAME["score_ragged"]


def test_targets_survive(eng, baseline):
    """installed targets, uniform and ragged, are read-only for every call that takes none"""
    uniform, ragged = _score_ops()
    for op in (uniform, ragged):
        first = _run(op, eng)                                         # installs its targets
        _same(op, first, baseline, "first score")
        for other in ops.NO_TARGET_OPS:
            _same(other, _run(other, eng), baseline, "between two %s calls" % op.name)
        again = _run(op, eng, installed=True)                               # no set_targets / set_targets_ragged
        assert ops.first_difference(op, again, first) is None, "%s: targets changed under %s" % (op.name, [o.name for o in ops.NO_TARGET_OPS])


def test_the_other_kind_of_targets_is_an_error():
    """a uniform call after only ragged targets were installed, and the reverse: an error code, not another length's pair table"""
    from desirna_amd import engine as E
    uniform, ragged = _score_ops()
    e = _engine()
    try:
        ragged.install(e)
        with pytest.raises(E.EngineError) as ei:
            e.score_batch(uniform.seqs)
        assert ei.value.code == BAD_ARG and "drna_set_targets" in str(ei.value)
        with pytest.raises(E.EngineError) as ei:
            e.ensemble_defect(uniform.seqs)
        assert ei.value.code == BAD_ARG and "drna_set_targets" in str(ei.value)
    finally:
        e.close()
    e = _engine()
    try:
        uniform.install(e)
        with pytest.raises(E.EngineError) as ei:
            e.score_ragged(ragged.seqs, list(range(len(ragged.seqs))))
        assert ei.value.code == BAD_ARG and "drna_set_targets_ragged" in str(ei.value)
        with pytest.raises(E.EngineError) as ei:
            e.ensemble_defect_ragged(ragged.seqs, list(range(len(ragged.seqs))))
        assert ei.value.code == BAD_ARG and "drna_set_targets_ragged" in str(ei.value)
    finally:
        e.close()


def _first_per_entry():
    """one operation per entry point that takes sequences as an argument of its own: the first of the table with three or more
    (the native loops take their sequences as in/out state and are not among them)"""
    seen = {}
    for op in ops.OPS:
        if not op.entry.startswith("drna_mc_run") and len(op.seqs) >= 3:
            seen.setdefault(op.entry, op)
    return list(seen.values())


def _with_x(seqs):
    bad = list(seqs)
    bad[2] = bad[2][:1] + "X" + bad[2][2:]
    return bad


def _too_long(seqs):
    """every sequence (ragged batches: the first) made one longer than the engine's max_L, strand A of a pair"""
    grow = lambda s: s[:1] + "A" * (ops.MAX_L + 1 - len(s.replace("&", ""))) + s[1:]
    if len({len(s) for s in seqs}) > 1:
        return [grow(seqs[0])] + list(seqs[1:])
    return [grow(s) for s in seqs]


@pytest.mark.parametrize("op", _first_per_entry(), ids=lambda op: op.entry)
def test_failed_call_leaves_no_trace(eng, baseline, op):
    from desirna_amd import engine as E
    op.install(eng)
    with pytest.raises(E.EngineError) as ei:
        _run(op, eng, installed=True, seqs=_with_x(op.seqs))
    assert ei.value.code == BAD_CHAR and "sequence 2 " in str(ei.value) + " ", str(ei.value)
    with pytest.raises((E.EngineError, ValueError)) as ei:
        _run(op, eng, installed=True, seqs=_too_long(op.seqs))
    assert not isinstance(ei.value, E.EngineError) or ei.value.code == BAD_ARG, str(ei.value)
    for after in (op, ops.BY_NAME["score_L200_R9"], ops.BY_NAME["sample_L100_S64"]):
        _same(after, _run(after, eng), baseline, "after a failed %s" % op.entry)


@pytest.mark.parametrize("name", ops.NAMES)
@pytest.mark.parametrize("byte", [0xFF, 0x00], ids=["ff", "00"])
def test_poisoned_workspaces(warm, baseline, byte, name):
    """poison, op -- and op, poison, op: every scratch buffer that exists holds the byte when the call starts"""
    op = ops.BY_NAME[name]
    warm.set_option("poison", byte)
    _same(op, _run(op, warm), baseline, "on workspaces of 0x%02X" % byte)
    warm.set_option("poison", byte)
    _same(op, _run(op, warm), baseline, "after itself and 0x%02X" % byte)


def test_poison_is_an_option_of_its_own(warm):
    from desirna_amd import engine as E
    for bad in (-1, 256):
        with pytest.raises(E.EngineError) as ei:
            warm.set_option("poison", bad)
        assert ei.value.code == BAD_ARG
