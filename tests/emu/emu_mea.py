"""ctypes loader for the TEST-ONLY CPU emulation of the MEA / centroid kernel (tests/emu/emu_mea.cpp -> libemu_mea.so: mea_kernel of
desirna_amd/csrc/fold_mea.hpp, unmodified, on hip_emu.h's stand-ins with the lanes of a workgroup as fibers of one OS thread)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_mea.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_mea.cpp", "emu_fibers.h", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_mea.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_mea.argtypes = [vp, ci, ci, ci, ci, ci, ci, C.c_char_p, vp, C.c_double, ci, vp, vp, vp, vp, vp, vp]
    return L


class EmuMea:
    def __init__(self, blob=None):
        self.L = build()
        self.blob = None if blob is None else np.ascontiguousarray(blob, dtype=np.int32)
        self.lds_max = self.L.emu_mea_lds_max()
        self.cand_lds = self.L.emu_mea_cand_lds()

    def run(self, P, gamma, seqs=None, cut=0, nt=64, lds=True, fill=0xFF):
        """P: (R, n+1, n+1) or (n+1, n+1); seqs (R strings without '&') switch the energies on.  -> dict(mea, cen: lists of str;
        val, dist: (R,); E: (R, 2) or None; ncand: (R,))"""
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.ndim == 2:
            P = P[None]
        R, n = P.shape[0], P.shape[1] - 1
        mea = np.zeros((R, n), dtype=np.uint8)
        cen = np.zeros((R, n), dtype=np.uint8)
        val = np.full(R, np.nan)
        dist = np.full(R, np.nan)
        E = np.full((R, 2), -7, dtype=np.int32) if seqs is not None else None
        nc = np.full(R, -7, dtype=np.int32)
        flat = None
        if seqs is not None:
            assert len(seqs) == R and all(len(s) == n for s in seqs) and self.blob is not None
            flat = "".join(seqs).encode()
        rc = self.L.emu_mea(self.blob.ctypes.data if self.blob is not None else None, 0 if self.blob is None else self.blob.size,
                            nt, 1 if lds else 0, R, n, cut, flat, P.ctypes.data, float(gamma), fill, mea.ctypes.data, val.ctypes.data,
                            cen.ctypes.data, dist.ctypes.data, None if E is None else E.ctypes.data, nc.ctypes.data)
        assert rc == 0, rc
        txt = lambda a: [row.tobytes().decode("ascii") for row in a]
        return dict(mea=txt(mea), cen=txt(cen), val=val, dist=dist, E=E, ncand=nc)
