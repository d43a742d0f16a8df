"""ctypes loader for the TEST-ONLY CPU emulation of the four auxiliary-fold kernels in their uniform and ragged forms
(tests/emu/emu_ragged_aux.cpp -> libemu_ragged_aux.so; the same hip_emu.h stand-ins as libemu.so).  The emulation spends its time
in the wave rendezvous, so jobs are spread over worker processes, one job per process at a time (the emulated __shared__ is a
function-local static)."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from tests.emu.emu import pair_table

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_ragged_aux.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")
KINDS = {"edef_lds": 0, "edef_general": 1, "subopt_lds": 2, "subopt_general": 3}


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_ragged_aux.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_ragged_aux.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_ragged_aux.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, C.c_char_p, vp, vp, vp, ci, vp, vp, vp, vp]
    return L


class EmuRaggedAux:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)

    def _call(self, kind, nt, ragged, R, L, lens, offs, idx, flat, pt, pt_off, tof, nblocks):
        ed = np.full(R, -1.0)
        E2 = np.full(R, -7, dtype=np.int32)
        E12 = np.full((R, 2), -7, dtype=np.int32)
        st = np.full(R, -7, dtype=np.int32)
        p = lambda a: a.ctypes.data if a is not None else None
        rc = self.L.emu_ragged_aux(self.blob.ctypes.data, self.blob.size, KINDS[kind], nt, int(ragged), R, L, p(lens), p(offs), p(idx),
                                   flat, p(pt), p(pt_off), p(tof), nblocks, p(ed), p(E2), p(E12), p(st))
        assert rc == 0
        return dict(edef=ed, E2=E2, E12=E12, status=st)

    def uniform(self, kind, seqs, target=None, nt=64):
        """equal-length sequences against one target (the ensemble-defect kinds), one workgroup after the other: the descriptors
        stay null.  Results are arrays over the sequences; what the kind does not write keeps its fill (-1.0 / -7)."""
        R, L = len(seqs), len(seqs[0])
        assert all(len(s) == L for s in seqs)
        pt = pair_table(target) if target is not None else None
        return self._call(kind, nt, False, R, L, None, None, None, "".join(seqs).encode(), pt, None, None, R)

    def ragged(self, kind, seqs, order, targets=None, max_L=None, nt=64, blocks=None):
        """ONE ragged launch: sequences of different lengths in one buffer, workgroup b -> sequence order[b], sequence r against
        targets[r] (one pair table per sequence, concatenated), the tables' pitch and slot size those of max_L.  `blocks`: run
        only the first so many workgroups of `order`."""
        R = len(seqs)
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int32)
        idx = np.array(order, dtype=np.int32)
        pt = pt_off = tof = None
        if targets is not None:
            tabs = [pair_table(t) for t in targets]
            pt = np.concatenate(tabs).astype(np.int16)
            pt_off = np.concatenate(([0], np.cumsum([t.size for t in tabs])[:-1])).astype(np.int32)
            tof = np.arange(R, dtype=np.int32)
        return self._call(kind, nt, True, R, int(max_L or lens.max()), lens, offs, idx, "".join(seqs).encode(), pt, pt_off, tof,
                          len(idx) if blocks is None else blocks)


_emu = None


def _job(job):
    """('uniform', kind, seqs, target, nt) or ('ragged', kind, seqs, order, targets, max_L, nt)"""
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuRaggedAux(params.load_blob())
    return _emu.uniform(*job[1:]) if job[0] == "uniform" else _emu.ragged(*job[1:])


def run_jobs(jobs, workers=16):
    """one job per worker process at a time, results in the order of jobs"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(jobs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_job, jobs))
