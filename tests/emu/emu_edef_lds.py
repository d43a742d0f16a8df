"""ctypes loader for the TEST-ONLY CPU emulation of the fused ensemble-defect kernel of short designs (tests/emu/emu_edef_lds.cpp ->
libemu_edef_lds.so; the same hip_emu.h stand-ins as libemu.so)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.emu.emu import _spawn_map, pair_table

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_edef_lds.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_edef_lds.cpp", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_edef_lds.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_edef_lds_max.argtypes = [ci]
    L.emu_edef_lds.argtypes = [vp, ci, ci, ci, ci, C.c_char_p, vp, ci, vp, vp, vp, vp]
    return L


class EmuEdefLds:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)
        self.max_one = self.L.emu_edef_lds_max(1)
        self.max_two = self.L.emu_edef_lds_max(0)

    def edef(self, seqs, target, nt=64, bpp_fill=0.0):
        """equal-length sequences ('AAAA', one strand) or pairs ('AAA&BBB') against one target -> (edef (R,), bpp (R, L+1, L+1)
        prefilled with bpp_fill, F4 (R, 4), status (R,))"""
        two = "&" in seqs[0]
        cut = seqs[0].index("&") if two else 0
        assert all(("&" in s) == two and (not two or s.index("&") == cut) and len(s) == len(seqs[0]) for s in seqs)
        flat = "".join(s.replace("&", "") for s in seqs).encode()
        R, L = len(seqs), len(seqs[0]) - int(two)
        pt = pair_table(target)
        assert pt.size == L + 2
        ed = np.zeros(R)
        bpp = np.full((R, L + 1, L + 1), bpp_fill)
        F4 = np.zeros((R, 4))
        st = np.zeros(R, dtype=np.int32)
        rc = self.L.emu_edef_lds(self.blob.ctypes.data, self.blob.size, R, L, cut, flat, pt.ctypes.data, nt, ed.ctypes.data,
                                 bpp.ctypes.data, F4.ctypes.data, st.ctypes.data)
        assert rc == 0
        return ed, bpp, F4, st


_emu = None


def _job(job):
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuEdefLds(params.load_blob())
    ed, bpp, F4, st = _emu.edef([job[0]], job[1], job[2], job[3])
    return float(ed[0]), bpp[0], F4[0], int(st[0])


def _any_job(job):
    """('lds', s, target, nt, fill): the fused kernel; ('general', s, target, nt): cofold_pf_kernel + cofold_outside_kernel of libemu.so"""
    if job[0] == "lds":
        return _job(job[1:])
    from tests.emu.emu import _edef_job
    return _edef_job(job[1:])


def run_jobs(jobs, workers=16):
    """mixed jobs for _any_job, one per worker process at a time, results in the order of jobs"""
    from tests.emu import emu
    build()
    emu.build()
    return _spawn_map(_any_job, jobs, workers)


def edef_lds_many(seqs, targets, nt=64, bpp_fill=0.0, workers=16):
    """one sequence or pair (with its own target) per worker process: [(edef, bpp, F4, status), ...] in the order of seqs"""
    build()
    return _spawn_map(_job, [(s, t, nt, bpp_fill) for s, t in zip(seqs, targets)], workers)
