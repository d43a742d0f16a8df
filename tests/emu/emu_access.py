"""ctypes loader for the TEST-ONLY CPU emulation of the partition function with positions held unpaired (tests/emu/emu_access.cpp ->
libemu_access.so: pf_kernel<NT, true> of desirna_amd/csrc/fold_pf.hpp and access_lds_kernel of fold_access.hpp, unmodified, on
hip_emu.h's stand-ins with the lanes of a workgroup as fibers of one OS thread)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu.emu import _spawn_map

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_access.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")

GENERAL_NT = (64, 128, 256)         # thread counts of pf_kernel<NT, true>
LDS_NT = (64, 128)                  # ... of access_lds_kernel


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_access.cpp", "emu_fibers.h", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_access.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_access.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, vp, ci, ci, ci, ci, vp, vp]
    return L


class EmuAccess:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)
        self.lds_max = self.L.emu_access_lds_max()

    def run(self, seqs, masks, nt=64, lds=False, masked=True, chunk=None):
        """equal-length sequences under each of the (M, L) masks -> (F (R, M) kcal/mol, status (R, M)).  lds: access_lds_kernel,
        else pf_kernel<NT, true>; masked=False (one all-zero mask): the unmasked pf_kernel<NT>; chunk: workgroups per launch
        (default: all of them in one)"""
        R, L = len(seqs), len(seqs[0])
        assert all(len(s) == L for s in seqs)
        m = np.ascontiguousarray(np.atleast_2d(masks), dtype=np.uint8)
        assert m.shape[1] == L
        M = m.shape[0]
        F = np.full((R, M), np.nan)
        st = np.full((R, M), -1, dtype=np.int32)
        rc = self.L.emu_access(self.blob.ctypes.data, self.blob.size, R, L, "".join(seqs).encode(), M, m.ctypes.data, nt, int(lds),
                               int(masked), int(chunk or R * M), F.ctypes.data, st.ctypes.data)
        assert rc == 0, rc
        return F, st


_emu = None


def _job(job):
    """(seqs, masks, nt, lds, masked, chunk) -> (F, status)"""
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuAccess(params.load_blob())
    return _emu.run(*job)


def lds_max():
    return build().emu_access_lds_max()


def run_jobs(jobs, workers=16):
    """jobs for _job, one per worker process at a time, results in the order of jobs"""
    build()
    return _spawn_map(_job, jobs, workers)
