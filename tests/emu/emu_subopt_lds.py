"""ctypes loader for the TEST-ONLY CPU emulation of the LDS-resident second-best kernels (tests/emu/emu_subopt_lds.cpp ->
libemu_subopt_lds.so; the same hip_emu.h stand-ins as libemu.so).  The emulation spends its time in the wave rendezvous, so
batches are spread over worker processes, one job per process at a time (the emulated __shared__ is a function-local static)."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_subopt_lds.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")
INF_REF = 10000000


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_subopt_lds.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_subopt_lds.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_subopt_lds.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, ci, ci, vp, vp, vp]
    return L


class EmuSuboptLds:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)
        self.max_len = self.L.emu_subopt_lds_max()
        self.lds_bytes = self.L.emu_subopt_lds_bytes()

    def second_best(self, seqs, lds=True, nt=64):
        """equal-length sequences, or 'AAA&BBB' pairs of equal strand lengths, in ONE batch -> (E2 (R,), E12 (R, 2), status (R,));
        lds=False: the general kernels"""
        cut = seqs[0].index("&") if "&" in seqs[0] else 0
        L = len(seqs[0]) - (1 if cut else 0)
        assert all(len(s) == len(seqs[0]) and (s.index("&") == cut if cut else "&" not in s) for s in seqs)
        R = len(seqs)
        flat = "".join(s.replace("&", "") for s in seqs).encode()
        E2 = np.zeros(R, dtype=np.int32)
        E12 = np.zeros((R, 2), dtype=np.int32)
        st = np.zeros(R, dtype=np.int32)
        rc = self.L.emu_subopt_lds(self.blob.ctypes.data, self.blob.size, R, L, cut, flat, nt, int(bool(lds)), E2.ctypes.data,
                                   E12.ctypes.data, st.ctypes.data)
        assert rc == 0
        return E2, E12, st


_emu = None


def _job(job):
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuSuboptLds(params.load_blob())
    E2, E12, st = _emu.second_best([job[0]], job[1], job[2])
    return int(E2[0]), (int(E12[0, 0]), int(E12[0, 1])), int(st[0])


def second_best_many(jobs, workers=16):
    """jobs: (sequence or pair, lds, nt), one per worker process at a time -> [(E2, (E1, E2nd), status), ...] in their order"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(jobs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_job, jobs))
