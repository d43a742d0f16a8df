"""The table of operations of tests/call_order_ops.py against the oracle alone (no GPU): the oracle accepts every input, and what
each anchor compares is finite and not degenerate -- a paired base in an MFE structure of the batch, a probability above 1e-3, a
pair joining the strands for the two-strand cases (asserted inside each operation's reference())."""
import numpy as np
import pytest

from tests import call_order_ops as ops


def _finite(x):
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_finite(v) for v in x)
    if isinstance(x, np.ndarray) and x.dtype.kind == "f":
        return bool(np.isfinite(x).all())
    return True


def test_table_shape():
    assert len(set(ops.NAMES)) == len(ops.OPS) >= 30
    entries = {op.entry for op in ops.OPS}
    assert len(entries) >= 20                                        # one operation at least per entry point of the table
    for op in ops.OPS:
        lens = [len(s.replace("&", "")) for s in op.seqs]
        assert 3 <= len(op.seqs) <= ops.MAX_R or op.name == "score_L200_R2", op.name
        assert max(lens) <= ops.MAX_L and sum(lens) <= ops.MAX_R * ops.MAX_L, op.name
        assert all(set(s) <= set("ACGU&") for s in op.seqs), op.name
        assert any(set(s) <= set("GC&") for s in op.seqs) or op.entry.startswith("drna_mc_run"), op.name       # the GC-only sequence
    assert {op.name for op in ops.NO_TARGET_OPS} >= {"subopt_L120", "structs_L100_K8", "sample_L100_S64", "mea_L200", "access_L100",
                                                     "self_dimer_L100"}


@pytest.mark.parametrize("name", ops.NAMES)
def test_inputs_and_reference(oracle, name):
    op = ops.BY_NAME[name]
    ref = op.reference(oracle)                                       # asserts that the inputs are not degenerate
    assert _finite(ref), name
    assert op.reference(oracle) is ref or ref is None                # computed once, shared by every test that needs it
