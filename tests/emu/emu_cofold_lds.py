"""ctypes loader for the TEST-ONLY CPU emulation of the short-pair co-fold kernels (tests/emu/emu_cofold_lds.cpp ->
libemu_cofold_lds.so; the same hip_emu.h stand-ins as libemu.so)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_cofold_lds.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_cofold_lds.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_cofold_lds.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_cofold_lds.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, ci, vp, vp, vp, vp]
    return L


class EmuCofoldLds:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)
        self.max_len = self.L.emu_cofold_lds_max()

    def cofold(self, seqs, nt=128):
        """'AAA&BBB' pairs of equal strand lengths -> (Emfe, structures with the '&', F4 (R, 4), status (2 R: MFE then PF))"""
        a0 = seqs[0].split("&")[0]
        cut, L = len(a0), len(seqs[0]) - 1
        assert all(len(s) == L + 1 and s.index("&") == cut for s in seqs)
        R = len(seqs)
        flat = "".join(s.replace("&", "") for s in seqs).encode()
        E = np.zeros(R, dtype=np.int32)
        ss = np.zeros((R, L), dtype=np.uint8)
        F4 = np.zeros((R, 4))
        st = np.zeros(2 * R, dtype=np.int32)
        rc = self.L.emu_cofold_lds(self.blob.ctypes.data, self.blob.size, R, L, cut, flat, nt, E.ctypes.data, ss.ctypes.data,
                                   F4.ctypes.data, st.ctypes.data)
        assert rc == 0
        return E, [bytes(r[:cut]).decode() + "&" + bytes(r[cut:]).decode() for r in ss], F4, st
