"""ctypes loader for the TEST-ONLY CPU emulation of the self-dimer partition function kernels (tests/emu/emu_self_dimer.cpp ->
libemu_self_dimer.so; the same hip_emu.h stand-ins as libemu.so)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_self_dimer.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_self_dimer.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_self_dimer.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_self_dimer.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci, vp, vp]
    return L


class EmuSelfDimer:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)
        self.lds_max = self.L.emu_self_dimer_lds_max()

    def fold(self, seqs, nt=128, lds=True):
        """equal-length sequences, each folded against itself -> (F4 (R, 4): FA, FB, FcAA, FAA in kcal/mol, status (R,));
        lds: the LDS-resident kernel, else the workspace kernel"""
        R, L = len(seqs), len(seqs[0])
        assert all(len(s) == L for s in seqs)
        F4 = np.zeros((R, 4))
        st = np.zeros(R, dtype=np.int32)
        rc = self.L.emu_self_dimer(self.blob.ctypes.data, self.blob.size, R, L, "".join(seqs).encode(), nt, int(bool(lds)),
                                   F4.ctypes.data, st.ctypes.data)
        assert rc == 0
        return F4, st
