"""The -sf term table (energy_scores.SF_TERMS): the batch scorer's sum against ScoreSeq.get_scoring_function on the record of the
same row, term by term, and the table's ids against Engine.TERM_IDS (no GPU: a hand-made engine, the native SimScore)."""
import numpy as np
import pytest

from desirna_amd import energy_scores as es
from desirna_amd import engine

TARGET = "((((....))))"
SEQS = ["GGGGAAAACCCC", "GCGCAAAAGCGC", "GGCGAUAACGCC"]
NAMES = ["Ed-Epf", "1-MCC", "sln_Epf", "Ed-MFE", "1-precision", "1-recall", "Edef"]          # ids 0..6 of mc_loop's switch


class HandMadeEngine:
    """R = 3, every array filled with distinct values; the three structures give three different sets of SimScore metrics"""
    Epf = np.array([-7.31, -3.07, -5.53])
    Emfe = np.array([-690, -250, -470], dtype=np.int32)
    ss = ["((((....))))", "(((.(..).)))", ".((.(...).))"]
    Ed = np.array([[-650], [-110], [-330]], dtype=np.int32)
    Edef = np.array([0.127, 3.91, 6.043])

    def score_batch_arrays(self, seqs_u8, flags=0):
        return self.Epf, self.Emfe, np.frombuffer("".join(self.ss).encode(), dtype=np.uint8).reshape(3, -1), self.Ed

    def ensemble_defect_arrays(self, seqs_u8):
        return self.Edef


@pytest.mark.parametrize("sf", [[(n, 1.0)] for n in NAMES] + [[(n, 0.3 + 0.37 * k) for k, n in enumerate(NAMES)]],
                         ids=NAMES + ["all"])
def test_batch_total_equals_the_records_scoring_function(sf):
    seqs = np.frombuffer("".join(SEQS).encode(), dtype=np.uint8).reshape(3, -1)
    b = es.score_arrays(HandMadeEngine(), engine.HostKernels(), TARGET, sf, seqs)
    assert len({tuple(x) for x in zip(b.mcc1, b.recall1, b.precision1)}) == 3 and b.mcc1[0] == 0
    assert len(set(b.score)) == 3
    for k in range(3):
        sc = es.record(b, k)
        assert sc.sequence == SEQS[k] and sc.mfe_ss == HandMadeEngine.ss[k] and sc.scoring_function == b.score[k]
        sc.get_scoring_function(sf)
        assert sc.scoring_function == b.score[k]


def test_term_ids_are_the_native_loops():
    assert [name for name, _, _ in es.SF_TERMS] == NAMES == es.AVAILABLE_SCORING_FUNCTIONS
    assert [i for _, i, _ in es.SF_TERMS] == list(range(7))
    assert engine.Engine.TERM_IDS == {name: i for name, i, _ in es.SF_TERMS}
    assert list(engine.Engine.TERM_IDS) == NAMES
