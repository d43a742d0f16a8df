"""ctypes loader for the TEST-ONLY CPU emulation of the K-best co-fold kernel (tests/emu/emu_cofold_kbest.cpp ->
libemu_cofold_kbest.so; the same hip_emu.h stand-ins as libemu.so).  The emulation spends its time in the wave rendezvous, so
batches are spread over worker processes, one job per process at a time (the emulated __shared__ is a function-local static)."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_cofold_kbest.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")
INF_REF = 10000000


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_cofold_kbest.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_cofold_kbest.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_cofold_kbest.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, ci, ci, vp, vp, vp]
    return L


class EmuCofoldKbest:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)

    def kbest(self, seqs, K, nt=128):
        """'AAA&BBB' pairs of equal strand lengths (or equal-length single strands: kbest_kernel) in ONE batch, as
        ``Engine.cofold_subopt_structs`` serves them: K = 1 .. 8 through the 4- / 8-list kernel -> (E (R, K), R lists of K
        strings with the '&' put back, status (R,))"""
        cut = seqs[0].index("&") if "&" in seqs[0] else 0
        L = len(seqs[0]) - (1 if cut else 0)
        assert all(len(s) == len(seqs[0]) and (s.index("&") == cut if cut else "&" not in s) for s in seqs)
        R, KT = len(seqs), 4 if K <= 4 else 8
        flat = "".join(s.replace("&", "") for s in seqs).encode()
        E = np.zeros((R, KT), dtype=np.int32)
        ss = np.zeros((R, KT, L), dtype=np.uint8)
        st = np.zeros(R, dtype=np.int32)
        rc = self.L.emu_cofold_kbest(self.blob.ctypes.data, self.blob.size, R, L, cut, flat, nt, KT, E.ctypes.data, ss.ctypes.data,
                                     st.ctypes.data)
        assert rc == 0
        strs = [[bytes(ss[r, k]).decode("ascii") for k in range(K)] for r in range(R)]
        if cut:
            strs = [[x[:cut] + "&" + x[cut:] for x in row] for row in strs]
        return E[:, :K].copy(), strs, st


_emu = None


def default_emu():
    """this process's emulator with the package's parameter blob"""
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuCofoldKbest(params.load_blob())
    return _emu


def cofold_kbest(seqs, K, nt=128):
    return default_emu().kbest(seqs, K, nt)


def _job(job):
    E, ss, st = cofold_kbest([job[0]], job[1], job[2])
    return [int(x) for x in E[0]], ss[0], int(st[0])


def cofold_kbest_many(jobs, workers=16):
    """jobs: (pair, K, nt), one per worker process at a time -> [(E list, strings, status), ...] in their order"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(jobs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_job, jobs))
