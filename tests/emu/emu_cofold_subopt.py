"""ctypes loader for the TEST-ONLY CPU emulation of cofold_subopt_kernel (tests/emu/emu_cofold_subopt.cpp), built into a
library of its own the way tests/emu/emu.py builds libemu.so.

The emulation spends its time waiting on the wave rendezvous, not computing, so batches are spread over worker processes
(each process holds its own copy of the kernel's static LDS; threads of one process would share it)."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_cofold_subopt.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")
INF_REF = 10000000


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_cofold_subopt.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_cofold_subopt.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_cofold_subopt.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, ci, vp, vp, vp]
    L.emu_cofold_subopt.restype = ci
    return L


_lib = None
_blob = None


def cofold_subopt(seqs, nt=128):
    """'A&B' strings of equal strand lengths -> (E2 (R,), E12 (R, 2), status (R,)), in this process"""
    global _lib, _blob
    if _lib is None:
        from desirna_amd import params
        _lib, _blob = build(), np.ascontiguousarray(params.load_blob(), dtype=np.int32)
    a0, b0 = seqs[0].split("&")
    cut, L, R = len(a0), len(a0) + len(b0), len(seqs)
    if any(len(s.split("&")[0]) != cut or len(s) != L + 1 for s in seqs):
        raise ValueError("all pairs of a batch must have the same strand lengths")
    E2 = np.zeros(R, dtype=np.int32)
    E12 = np.zeros((R, 2), dtype=np.int32)
    st = np.zeros(R, dtype=np.int32)
    rc = _lib.emu_cofold_subopt(_blob.ctypes.data, _blob.size, R, L, cut, "".join(s.replace("&", "") for s in seqs).encode(), nt,
                                E2.ctypes.data, E12.ctypes.data, st.ctypes.data)
    assert rc == 0
    return E2, E12, st


def _one(job):
    seq, nt = job
    E2, E12, st = cofold_subopt([seq], nt)
    return int(E2[0]), (int(E12[0, 0]), int(E12[0, 1])), int(st[0])


def cofold_subopt_many(seqs, nt=128, workers=16):
    """one pair per job, spread over worker processes: [(E2, (E1, E2nd), status), ...] in the order of seqs"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(seqs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_one, [(s, nt) for s in seqs]))
