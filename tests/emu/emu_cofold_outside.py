"""ctypes loader for the TEST-ONLY CPU emulation of cofold_pf_kernel + cofold_outside_kernel (tests/emu/emu_cofold_outside.cpp),
built into a library of its own the way tests/emu/emu_cofold_subopt.py builds its library.

The emulation spends its time waiting on the wave rendezvous, not computing, so batches are spread over worker processes
(each process holds its own copy of the kernels' static LDS; threads of one process would share it)."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_cofold_outside.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_cofold_outside.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_cofold_outside.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_cofold_edef.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, vp, ci, vp, vp, vp, vp]
    L.emu_cofold_edef.restype = ci
    return L


def pair_table(target):
    """1-based partner table (L + 2 int16, 0 = unpaired) of a dot-bracket target; '&' removed, '(' ')' pairs only"""
    target = target.replace("&", "")
    pt = np.zeros(len(target) + 2, dtype=np.int16)
    stk = []
    for i, ch in enumerate(target, 1):
        if ch == "(":
            stk.append(i)
        elif ch == ")":
            o = stk.pop()
            pt[o], pt[i] = i, o
    return pt


_lib = None
_blob = None


def cofold_edef(seqs, target, nt=128):
    """'A&B' strings of equal strand lengths, one target -> (edef (R,), bpp (R, L+1, L+1), F4 (R, 4), status (R,)), in this
    process; the pairs go through one workspace slot one after the other"""
    global _lib, _blob
    if _lib is None:
        from desirna_amd import params
        _lib, _blob = build(), np.ascontiguousarray(params.load_blob(), dtype=np.int32)
    a0, b0 = seqs[0].split("&")
    cut, L, R = len(a0), len(a0) + len(b0), len(seqs)
    if any(len(s.split("&")[0]) != cut or len(s) != L + 1 for s in seqs):
        raise ValueError("all pairs of a batch must have the same strand lengths")
    pt = pair_table(target)
    assert pt.size == L + 2
    ed = np.zeros(R)
    bpp = np.zeros((R, L + 1, L + 1))
    F4 = np.zeros((R, 4))
    st = np.zeros(R, dtype=np.int32)
    rc = _lib.emu_cofold_edef(_blob.ctypes.data, _blob.size, R, L, cut, "".join(s.replace("&", "") for s in seqs).encode(),
                              pt.ctypes.data, nt, ed.ctypes.data, bpp.ctypes.data, F4.ctypes.data, st.ctypes.data)
    assert rc == 0
    return ed, bpp, F4, st


def _one(job):
    seq, target, nt = job
    ed, bpp, F4, st = cofold_edef([seq], target, nt)
    return float(ed[0]), bpp[0], F4[0], int(st[0])


def cofold_edef_many(seqs, targets, nt=128, workers=16):
    """one pair (with its own target) per job, spread over worker processes: [(edef, bpp, F4, status), ...] in the order of seqs"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(seqs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_one, [(s, t, nt) for s, t in zip(seqs, targets)]))
