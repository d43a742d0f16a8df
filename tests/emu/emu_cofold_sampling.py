"""ctypes loader for the TEST-ONLY CPU emulation of the two-strand stochastic traceback (tests/emu/emu_cofold_sampling.cpp ->
libemu_cofold_sampling.so: cofold_pf_kernel + cofold_columns_kernel + cofold_sample_kernel, unmodified, on hip_emu.h's stand-ins
with the lanes of a workgroup as fibers of one OS thread).  A launch is R x G workgroups; the jobs of run_jobs are ranges of its
workgroups, run side by side in worker processes, one job per process at a time (the emulated __shared__ is a function-local
static).  Pairs are 'AAAA&BBBB' strings, all of one launch with the same two lengths."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libemu_cofold_sampling.so")
_CSRC = os.path.join(_HERE, "..", "..", "desirna_amd", "csrc")


def build():
    srcs = [os.path.join(_HERE, f) for f in ("emu_cofold_sampling.cpp", "emu_fibers.h", "hip_emu.h", "hip_emu_prims.h")]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", _HERE, "-o", _LIB,
                               os.path.join(_HERE, "emu_cofold_sampling.cpp")])
    L = C.CDLL(_LIB)
    vp, ci = C.c_void_p, C.c_int
    L.emu_cofold_sample.argtypes = [vp, ci, ci, ci, ci, ci, C.c_char_p, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    return L


def seeds_of(seed, R):
    """an integer seed gives pair r the seed seed + r (mod 2^64); an array gives the seeds themselves"""
    if np.ndim(seed) == 0:
        return np.array([(int(seed) + r) % (1 << 64) for r in range(R)], dtype=np.uint64)
    out = np.ascontiguousarray(seed, dtype=np.uint64)
    assert out.shape == (R,)
    return out


def split_pairs(pairs):
    """['A&B', ...] -> (flat strings, cut); every pair with the same two lengths"""
    cut = pairs[0].index("&")
    flat = [p.replace("&", "") for p in pairs]
    assert all(p.count("&") == 1 and p.index("&") == cut and len(f) == len(flat[0]) for p, f in zip(pairs, flat))
    return flat, cut


class EmuCofoldSampling:
    def __init__(self, blob):
        self.L = build()
        self.blob = np.ascontiguousarray(blob, dtype=np.int32)

    def raw(self, pairs, S, seed=0, nt=64, G=1, blocks=None, fill=0xFF):
        """workgroups blocks = (b0, b1) of the launch (None: all R x G) -> dict(ss uint8 (R, S, L), E int32 (R, S), F4 (R, 4),
        status (R,), cut); what these workgroups do not write keeps its fill: 0 in ss, -7 in E and status, nan in F4.  fill: the byte the
        workspace slot and the columns hold before the kernels run (0xFF: NaN)"""
        flat, cut = split_pairs(pairs)
        R, L = len(flat), len(flat[0])
        sd = seeds_of(seed, R)
        ss = np.zeros((R, S, L), dtype=np.uint8)
        E = np.full((R, S), -7, dtype=np.int32)
        F4 = np.full((R, 4), np.nan)
        st = np.full(R, -7, dtype=np.int32)
        b0, b1 = (0, R * G) if blocks is None else blocks
        rc = self.L.emu_cofold_sample(self.blob.ctypes.data, self.blob.size, nt, R, L, cut, "".join(flat).encode(), sd.ctypes.data,
                                      S, G, b0, b1, fill, ss.ctypes.data, E.ctypes.data, F4.ctypes.data, st.ctypes.data)
        assert rc == 0, rc
        return dict(ss=ss, E=E, F4=F4, status=st, cut=cut)


def strings(ss, cut=None):
    """uint8 (..., S, L) -> nested lists of str, the '&' put back at cut when given; a sample nobody wrote is ''"""
    if ss.ndim == 3:
        return [strings(x, cut) for x in ss]
    raw = ss.tobytes().decode("ascii")
    L = ss.shape[1]
    out = [raw[k * L:(k + 1) * L].rstrip("\0") for k in range(ss.shape[0])]
    return out if cut is None else [s[:cut] + "&" + s[cut:] if s else s for s in out]


_emu = None


def _job(job):
    """(pairs, S, seed, nt, G, blocks[, fill])"""
    global _emu
    if _emu is None:
        from desirna_amd import params
        _emu = EmuCofoldSampling(params.load_blob())
    return _emu.raw(*job)


def run_jobs(jobs, workers=8):
    """one job per worker process at a time, results in the order of jobs"""
    build()                                       # compile once, before the workers load the library
    n = max(1, min(workers, 2 * (os.cpu_count() or 1), len(jobs)))
    with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(_job, jobs))


def merge(parts):
    """results of jobs over disjoint workgroups of ONE launch -> one result (every cell from the job that wrote it)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in parts[0].items()}
    for p in parts[1:]:
        w = p["ss"].any(axis=2)
        out["ss"][w] = p["ss"][w]
        out["E"][w] = p["E"][w]
        t = p["status"] != -7
        out["status"][t] = p["status"][t]
        out["F4"][t] = p["F4"][t]
    return out


def launch_jobs(pairs, S, seed=0, nt=64, G=8):
    """the jobs of one launch of len(pairs) x G workgroups, one workgroup each"""
    return [(list(pairs), S, seed, nt, G, (b, b + 1)) for b in range(len(pairs) * G)]


def sample_many(cases, nt=64, G=8, workers=8):
    """cases: [(pairs, S, seed), ...], each a launch of its own, all their workgroups side by side -> one merged result per case"""
    jobs, owner = [], []
    for c, (pairs, S, seed) in enumerate(cases):
        js = launch_jobs(pairs, S, seed, nt, G)
        jobs += js
        owner += [c] * len(js)
    res = run_jobs(jobs, workers)
    return [merge([r for r, o in zip(res, owner) if o == c]) for c in range(len(cases))]
