"""ctypes binding of the gfx950 scoring engine (include/desirna_amd.h -> libdesirna_amd.so).

This is the Python side of the drop-in boundary: what the reference gets from the ViennaRNA SWIG
module per sequence (``RNA.fold_compound(seq, md).pf() / .mfe() / .eval_structure()``, reference
``utils/energy_scores.py:147-151,75``) is obtained here for a whole batch of replicas per call.
There is deliberately NO CPU fallback: if the HIP library is missing or no GPU is present the
constructor raises.
"""
import ctypes as C
import os

import numpy as np

from . import params as _params

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdesirna_amd.so")

NEED_PF, NEED_MFE, NEED_PK, NEED_EVAL = 1, 2, 4, 8

_ERRORS = {-1: "bad argument", -2: "bad parameter blob", -3: "HIP/device error", -4: "bad sequence character",
           -5: "unbalanced structure", -6: "partition function out of fp64 range", -7: "internal (traceback)"}

_vp, _ci, _u32, _dbl, _str = C.c_void_p, C.c_int, C.c_uint32, C.c_double, C.c_char_p
# every export of include/desirna_amd.h: name -> (restype, argtypes)
_SIGNATURES = {
    "drna_abi_version": (_ci, []),
    "drna_create": (_ci, [_vp, _ci, _ci, _ci, _ci, C.POINTER(_vp)]),
    "drna_destroy": (None, [_vp]),
    "drna_last_error": (_str, [_vp]),
    "drna_set_targets": (_ci, [_vp, _ci, _ci, _str]),
    "drna_score_batch": (_ci, [_vp, _ci, _ci, _str, _u32, _vp, _vp, _vp, _vp]),
    "drna_score_batch_device": (_ci, [_vp, _ci, _ci, _vp, _u32, _vp, _vp, _vp, _vp]),
    "drna_last_timing": (_ci, [_vp, _vp]),
    "drna_info": (_ci, [_vp, _vp]),
    "drna_timing_sums": (_ci, [_vp, _vp, _ci]),
    "drna_set_option": (_ci, [_vp, _str, _ci]),
    "drna_get_option": (_ci, [_vp, _str, _vp]),
    "drna_debug_strip_clocks": (_ci, [_vp, _vp, _ci]),
    "drna_ensemble_defect_batch": (_ci, [_vp, _ci, _ci, _str, _vp, _vp]),
    "drna_ensemble_defect_batch_device": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp]),
    "drna_last_edef_timing": (_ci, [_vp, _vp]),
    "drna_set_targets_ragged": (_ci, [_vp, _ci, _vp, _str]),
    "drna_score_ragged": (_ci, [_vp, _ci, _vp, _str, _vp, _u32, _vp, _vp, _vp, _vp]),
    "drna_cofold_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _u32, _vp, _vp, _vp, _vp]),
    "drna_mc_run": (_ci, [_vp, _ci, _ci, _ci, _str, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci, _vp,
                          _dbl, _ci, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_subopt_energy_batch": (_ci, [_vp, _ci, _ci, _str, _vp, _vp]),
    "drna_cofold_subopt_energy_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _vp, _vp]),
    "drna_cofold_ensemble_defect_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _vp, _vp]),
    "drna_subopt_structs_batch": (_ci, [_vp, _ci, _ci, _str, _ci, _vp, _vp]),
    "drna_cofold_subopt_structs_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _ci, _vp, _vp]),
    "drna_simscore_batch": (_ci, [_ci, _ci, _str, _vp, _vp, _vp, _vp]),
    "drna_propose_batch": (_ci, [_ci, _ci, _str, _vp, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci, _vp, _vp]),
    "drna_propose_batch_alt": (_ci, [_ci, _ci, _str, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci,
                                     _vp, _vp]),
    "drna_metropolis_batch": (_ci, [_ci, _vp, _vp, _vp, _dbl, _vp, _vp, _vp]),
    "drna_propose_batch_co": (_ci, [_ci, _ci, _str, _vp, _ci, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci, _vp, _vp]),
    "drna_mc_run_cofold": (_ci, [_vp, _ci, _ci, _ci, _ci, _str, _vp, _ci, _vp, _ci, _dbl, _dbl, _ci, _vp, _dbl, _ci, _vp, _vp, _vp,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_mc_run_nd": (_ci, [_vp, _ci, _ci, _ci, _str, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci, _vp,
                             _dbl, _ci, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_mc_run_cofold_nd": (_ci, [_vp, _ci, _ci, _ci, _ci, _str, _vp, _ci, _vp, _ci, _dbl, _dbl, _ci, _vp, _dbl, _ci, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_self_dimer_batch": (_ci, [_vp, _ci, _ci, _str, _vp, _vp]),
    "drna_mc_run_oa": (_ci, [_vp, _ci, _ci, _ci, _str, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _dbl, _dbl, _ci, _vp,
                             _dbl, _ci, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_mc_run_ragged": (_ci, [_vp, _ci, _vp, _vp, _ci, _str, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _dbl, _ci, _vp, _vp, _u32, _vp,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_ensemble_defect_ragged": (_ci, [_vp, _ci, _vp, _str, _vp, _vp]),
    "drna_subopt_energy_ragged": (_ci, [_vp, _ci, _vp, _str, _vp, _vp]),
    "drna_mc_run_ragged_nd": (_ci, [_vp, _ci, _vp, _vp, _ci, _str, _vp, _vp, _vp, _dbl, _dbl, _ci, _vp, _dbl, _ci, _vp, _vp, _u32, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_motif_score_batch": (_ci, [_ci, _ci, _vp, _ci, _vp, _str, _vp, _vp]),
    "drna_set_motifs": (_ci, [_vp, _ci, _vp, _str, _vp]),
    "drna_rng_seed": (_ci, [_ci, _vp, _vp]),
    "drna_rng_random": (_ci, [_ci, _vp, _vp]),
    "drna_sample_structures_batch": (_ci, [_vp, _ci, _ci, _str, _ci, _vp, _vp, _vp, _vp]),
    "drna_cofold_sample_structures_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _ci, _vp, _vp, _vp, _vp]),
    "drna_mea_structures_batch": (_ci, [_vp, _ci, _ci, _str, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_cofold_mea_structures_batch": (_ci, [_vp, _ci, _ci, _ci, _str, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "drna_last_mea_timing": (_ci, [_vp, _vp]),
    "drna_pf_unpaired_batch": (_ci, [_vp, _ci, _ci, _str, _ci, _vp, _vp]),
    "drna_last_access_timing": (_ci, [_vp, _vp]),
}
EXPORTS = tuple(_SIGNATURES)

ABI_VERSION = 3        # DRNA_ABI_VERSION this binding was written against (include/desirna_amd.h)

RNG_WORDS = 625        # DRNA_RNG_WORDS: uint32 words of one replica's MT19937 stream

OLIGO_STATES = {"heterodimer": 1, "homodimer": 2}      # oligo_state of drna_propose_batch_co / drna_mc_run_cofold


def co_allowed_mask(prob):
    """allowed-letter mask of a design.DesignProblem for the native proposers: bit0 A .. bit3 U, 0 for the '&' column of two strands"""
    return np.array([sum(1 << "ACGU".index(c) for c in a if c != "&") for a in prob.allowed], dtype=np.uint8)


def _packed(prob):
    """the arrays of HostKernels._pack, made on first use"""
    if getattr(prob, "_native_pack", None) is None:
        HostKernels._pack(prob)
    return prob._native_pack


def _motif_arrays(motifs):
    """motifs -- an ordered mapping key -> value (or key -> (compiled regex, value), what ``energy_scores.parse_motifs`` returns)
    or a list of (key, value); a repeated key keeps its first position and takes its last value, as in a dict; None or empty:
    no motifs -- -> (count, int32 lengths, the keys concatenated as bytes, float64 values) of drna_set_motifs /
    drna_motif_score_batch.  A key outside ASCII can be no motif: bytes the library refuses."""
    d = {}
    for key, v in (motifs.items() if hasattr(motifs, "items") else motifs or ()):
        d[key] = float(v[1] if isinstance(v, tuple) else v)
    keys = [k.encode("ascii", "replace") for k in d]
    return (len(d), np.array([len(k) for k in keys] or [0], dtype=np.int32), b"".join(keys),
            np.array(list(d.values()) or [0.0], dtype=np.float64))


def _check_rng(rng_state, R):
    assert rng_state.dtype == np.uint32 and rng_state.shape == (R, RNG_WORDS) and rng_state.flags.c_contiguous


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("desirna_amd engine error %d (%s): %s" % (code, _ERRORS.get(code, "?"), msg))
        self.code = code


def load_library(path=None):
    """dlopen the C-ABI library and declare its signatures (raises if it has not been built)."""
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C desirna_amd/csrc`); there is no CPU fallback" % path)
    L = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():         # drna_abi_version first: nothing else is called before the check
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
        if name == "drna_abi_version" and fn() != ABI_VERSION:
            raise EngineError(-1, "library ABI version %d, this binding expects %d: rebuild desirna_amd/csrc" % (fn(), ABI_VERSION))
    return L


def _equal_length(seqs):
    """(R, L) of a batch of equal-length sequences"""
    R, L = len(seqs), len(seqs[0])
    if any(len(s) != L for s in seqs):
        raise ValueError("all sequences of a batch must have the same length")
    return R, L


def _as_u8(seqs):
    """list of equal-length strings -> (R, L) uint8 array of their ASCII letters"""
    return np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8).reshape(_equal_length(seqs))


def _split_pairs(seqs):
    """'AAAA&BBBB' strings of the same strand lengths -> (both strands of every pair in one bytes object, R, L, cut)"""
    a0, b0 = seqs[0].split("&")
    cut, L = len(a0), len(a0) + len(b0)
    flat = []
    for s in seqs:
        a, b = s.split("&")
        if len(a) != cut or len(a) + len(b) != L:
            raise ValueError("all pairs of a batch must have the same strand lengths")
        flat.append(a + b)
    return "".join(flat).encode("ascii"), len(flat), L, cut


KT = 0.001987204259 * (273.15 + 37)      # kcal/mol: the kT of energy_scores.kTlog_* (boltzmann constant x the model's 37 degC)


def mask_array(masks, L):
    """masks of :meth:`Engine.unpaired_free_energy` -> (M, L) uint8, 1 = the position stays unpaired.  `masks`: an (M, L) (or one
    (L,)) uint8 / bool array, one string or a list of strings over 'x' (stays unpaired) and '.'"""
    if isinstance(masks, str):
        masks = [masks]
    if len(masks) and isinstance(masks[0], str):
        for m in masks:
            bad = set(m) - set("x.")
            if bad:
                raise ValueError("mask %r: character %r (a mask holds 'x' and '.' only)" % (m, sorted(bad)[0]))
            if len(m) != L:
                raise ValueError("mask %r: %d characters for sequences of %d" % (m, len(m), L))
        return np.array([[c == "x" for c in m] for m in masks], dtype=np.uint8).reshape(len(masks), L)
    a = np.atleast_2d(np.asarray(masks))
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != L:
        raise ValueError("masks must be (M, %d), M >= 1; got %r" % (L, a.shape))
    return np.ascontiguousarray(a != 0, dtype=np.uint8)


def _sample_seeds(seed, R):
    """the seed rule of the samplers: an integer gives sequence r the seed seed + r (mod 2^64), an array the R seeds themselves"""
    if np.ndim(seed) == 0:
        return np.array([(int(seed) + r) % (1 << 64) for r in range(R)], dtype=np.uint64)
    seeds = np.ascontiguousarray(seed, dtype=np.uint64)
    if seeds.shape != (R,):
        raise ValueError("seed must be an integer or one uint64 per sequence")
    return seeds


_LIVE = None          # weak set of open engines, _CLOSED_FALLBACKS: the counters of the closed ones (sync_fallbacks_total)
_CLOSED_FALLBACKS = 0


def sync_fallbacks_total():
    """Calls of this process, over all engines, in which a fold by several workgroups lost a partner and was redone with one
    workgroup per fold (``drna_get_option("sync_fallbacks")``): 0 on a healthy box; the GPU test suite asserts it."""
    return _CLOSED_FALLBACKS + sum(e.get_option("sync_fallbacks") for e in list(_LIVE or ()) if e._h and e._h.value)


class Engine:
    """One engine per GPU (``RNA.params_load`` + all ``RNA.fold_compound`` allocations, done once)."""

    def __init__(self, max_R, max_L, device=0, params="1999", lib=None):
        self._L = load_library(lib)
        self._h = C.c_void_p()
        blob = params if isinstance(params, np.ndarray) else _params.load_params(params)
        blob = np.ascontiguousarray(blob, dtype=np.int32)
        rc = self._L.drna_create(blob.ctypes.data, blob.size, int(device), int(max_R), int(max_L), C.byref(self._h))
        if rc != 0:
            raise EngineError(rc, self._L.drna_last_error(None).decode())
        self.max_R, self.max_L, self.device = int(max_R), int(max_L), int(device)
        self.n_targets = 0
        self.L = None
        global _LIVE
        if _LIVE is None:
            import weakref
            _LIVE = weakref.WeakSet()
        _LIVE.add(self)

    def set_option(self, name, value):
        """Engine option (``drna_set_option``): ``"dual"`` = fold small batches with two workgroups per sequence (default on).
        ``"poison"`` (tests) fills every scratch buffer the engine holds with the byte `value`; no result may depend on it."""
        self._check(self._L.drna_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        """Reads an option back, or the counter ``"sync_fallbacks"`` (``drna_get_option``)."""
        v = C.c_int(0)
        self._check(self._L.drna_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            global _CLOSED_FALLBACKS
            try:
                _CLOSED_FALLBACKS += self.get_option("sync_fallbacks")
            except Exception:
                pass
            self._L.drna_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._L.drna_last_error(self._h).decode())

    def set_targets(self, targets):
        """targets[0] = design target, targets[1:] = alternative structures ('&' already removed)."""
        targets = list(targets)
        L = len(targets[0]) if targets else 1
        if any(len(t) != L for t in targets):
            raise ValueError("all target structures must have the same length")
        self._check(self._L.drna_set_targets(self._h, len(targets), L, "".join(targets).encode("ascii")))
        self.n_targets, self.L = len(targets), L

    def set_motifs(self, motifs):
        """Sequence motifs (``-motifs``; drna_set_motifs) of every ``mc_run*`` call from now on: each proposal whose string holds
        a motif gets the motif's value added to its score, last of all additions.  `motifs`: an ordered mapping key -> value
        (``energy_scores.parse_motifs``'s dict is one) or a list of (key, value); None or empty clears the set.  It is engine
        state: whoever shares an engine between runs sets it before each run.  ``get_option("motifs")`` is the count."""
        n, lens, keys, values = _motif_arrays(motifs)
        self._check(self._L.drna_set_motifs(self._h, n, lens.ctypes.data, keys, values.ctypes.data))

    def score_batch(self, seqs, flags=NEED_PF | NEED_MFE | NEED_EVAL):
        """String form of :meth:`score_batch_arrays`: seqs is a list of equal-length strings.  Returns dict(Epf, Emfe, mfe_ss, Ed)
        (None if not requested); energies in ViennaRNA's units: Epf kcal/mol (float), Emfe / Ed int dcal/mol."""
        Epf, Emfe, ss, Ed = self.score_batch_arrays(_as_u8(seqs), flags)
        want_mfe = flags & (NEED_MFE | NEED_PK)
        return {"Epf": Epf if flags & NEED_PF else None, "Emfe": Emfe if want_mfe else None,
                "mfe_ss": [bytes(r).decode("ascii") for r in ss] if want_mfe else None, "Ed": Ed if flags & NEED_EVAL else None}

    def score_batch_arrays(self, seqs_u8, flags=NEED_PF | NEED_MFE | NEED_EVAL):
        """Array form for hot host loops: seqs_u8 is an (R, L) uint8 array of ASCII letters; returns
        (Epf float64[R], Emfe int32[R], mfe_ss uint8[R, L], Ed int32[R, n_targets]) without building Python strings."""
        seqs_u8 = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
        R, L = seqs_u8.shape
        Epf = np.zeros(R, dtype=np.float64)
        Emfe = np.zeros(R, dtype=np.int32)
        ss = np.zeros((R, L), dtype=np.uint8)
        Ed = np.zeros((R, max(1, self.n_targets)), dtype=np.int32)
        self._check(self._L.drna_score_batch(self._h, R, L, seqs_u8.ctypes.data_as(C.c_char_p), flags,
                                             Epf.ctypes.data, Emfe.ctypes.data, ss.ctypes.data, Ed.ctypes.data))
        return Epf, Emfe, ss, Ed

    def score_batch_device(self, d_seqs, R, L, flags, d_Epf=None, d_Emfe=None, d_ss=None, d_Ed=None):
        """Device-resident variant: arguments are raw device pointers (e.g. ``tensor.data_ptr()``).
        The caller must have made the inputs visible (``torch.cuda.synchronize()``) before the call."""
        self._check(self._L.drna_score_batch_device(self._h, R, L, d_seqs, flags, d_Epf, d_Emfe, d_ss, d_Ed))

    def set_targets_ragged(self, structures):
        """Structures of different lengths for :meth:`score_ragged` ('&' already removed)."""
        lens = np.array([len(t) for t in structures], dtype=np.int32)
        self._check(self._L.drna_set_targets_ragged(self._h, len(structures), lens.ctypes.data, "".join(structures).encode("ascii")))
        self.n_ragged_targets = len(structures)

    def score_ragged(self, seqs, target_of=None, flags=NEED_PF | NEED_MFE | NEED_EVAL):
        """String form of :meth:`score_ragged_arrays`: sequences of DIFFERENT lengths in one call (BASELINE config 4: many
        puzzles x replicas).  target_of[r] is the index (into :meth:`set_targets_ragged`) of the structure sequence r is
        evaluated on.  Returns dict(Epf, Emfe, mfe_ss, Ed[R])."""
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        Epf, Emfe, ss, Ed = self.score_ragged_arrays(np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8), lens, target_of, flags)
        out_ss = None
        if ss is not None:
            b = ss.tobytes().decode("ascii")
            offs = np.concatenate(([0], np.cumsum(lens)))
            out_ss = [b[offs[k]:offs[k + 1]] for k in range(len(lens))]
        return {"Epf": Epf, "Emfe": Emfe, "mfe_ss": out_ss, "Ed": Ed}

    def score_ragged_arrays(self, flat_u8, lens, target_of=None, flags=NEED_PF | NEED_MFE | NEED_EVAL):
        """Array form for hot host loops: flat_u8 holds the letters of all sequences back to back (uint8, sum(lens)), lens their
        lengths.  Returns (Epf float64[R], Emfe int32[R], mfe_ss uint8[sum(lens)] laid out like flat_u8, Ed int32[R]); None for
        what `flags` does not ask for (Ed also without target_of)."""
        flat_u8 = np.ascontiguousarray(flat_u8, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        R, total = len(lens), int(lens.sum())
        if flat_u8.shape != (total,):
            raise ValueError("flat_u8 must hold sum(lens) letters")
        if target_of is None:
            flags &= ~NEED_EVAL
        tof = np.ascontiguousarray(target_of, dtype=np.int32) if target_of is not None else None
        if tof is not None and tof.shape != (R,):
            raise ValueError("target_of must name one structure per sequence")
        Epf = np.zeros(R, dtype=np.float64) if flags & NEED_PF else None
        want_mfe = flags & (NEED_MFE | NEED_PK)
        Emfe = np.zeros(R, dtype=np.int32) if want_mfe else None
        ss = np.zeros(total, dtype=np.uint8) if want_mfe else None
        Ed = np.zeros(R, dtype=np.int32) if flags & NEED_EVAL else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self._L.drna_score_ragged(self._h, R, lens.ctypes.data, flat_u8.ctypes.data_as(C.c_char_p), ptr(tof), flags,
                                              ptr(Epf), ptr(Emfe), ptr(ss), ptr(Ed)))
        return Epf, Emfe, ss, Ed

    def cofold_batch(self, seqs, flags=NEED_PF | NEED_MFE | NEED_EVAL):
        """Two-strand scoring: seqs are 'AAAA&BBBB' strings with the same strand lengths.  Returns dict(FA, FB, FcAB, FAB
        (kcal/mol; the reference's Epf is FAB), Emfe (dcal/mol), mfe_ss (with the '&' re-inserted), Ed (vs. set_targets))."""
        flat, R, L, cut = _split_pairs(seqs)
        if not (flags & NEED_EVAL and self.n_targets):
            flags &= ~NEED_EVAL
        F4 = np.zeros((R, 4), dtype=np.float64) if flags & NEED_PF else None
        Emfe = np.zeros(R, dtype=np.int32) if flags & NEED_MFE else None
        ss = np.zeros((R, L), dtype=np.uint8) if flags & NEED_MFE else None
        Ed = np.zeros((R, max(1, self.n_targets)), dtype=np.int32) if flags & NEED_EVAL else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self._L.drna_cofold_batch(self._h, R, L, cut, flat, flags, ptr(F4), ptr(Emfe),
                                              ptr(ss), ptr(Ed)))
        out = {"Emfe": Emfe, "Ed": Ed, "mfe_ss": None, "FA": None, "FB": None, "FcAB": None, "FAB": None}
        if ss is not None:
            out["mfe_ss"] = [bytes(r[:cut]).decode() + "&" + bytes(r[cut:]).decode() for r in ss]
        if F4 is not None:
            out.update(FA=F4[:, 0], FB=F4[:, 1], FcAB=F4[:, 2], FAB=F4[:, 3])
        return out

    TERM_IDS = {"Ed-Epf": 0, "1-MCC": 1, "sln_Epf": 2, "Ed-MFE": 3, "1-precision": 4, "1-recall": 5, "Edef": 6}

    def _mc_run(self, name, head, mid, keys, n_vals, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, rng_state,
                state, counters, best, L_const, subopt_e, oa=False):
        """drna_mc_run / drna_mc_run_cofold (`name`; with `subopt_e` their _nd forms): `head` are the arguments between R and the
        shelf indices, `mid` those between the term weights and the random streams, `keys` the arrays of `state` in call order.
        `oa`: drna_mc_run_oa, which takes subopt_e (or NULL), then the state's oligo_fraction and bonus, after `best`"""
        R = state["seqs"].shape[0]
        nd = subopt_e is not None
        _check_rng(rng_state, R)
        assert best["vals"].shape == (n_vals + nd,)
        ids = np.array([self.TERM_IDS[n] for n, _ in scoring_f], dtype=np.int32)
        ws = np.array([w for _, w in scoring_f], dtype=np.float64)
        sh = np.ascontiguousarray(shelf_index, dtype=np.int32)
        tt = np.ascontiguousarray(temps, dtype=np.float64)
        p = lambda a: a.ctypes.data
        args = [self._h, R] + head + [p(sh), int(n_shelves), float(tm_max), float(tm_min), int(bool(targeted)), p(tt), float(L_const),
                                      len(ids), p(ids), p(ws)] + mid + [p(rng_state)] + [p(state[k]) for k in keys] + [
                                          p(counters), p(best["seq"]), p(best["ss"]), p(best["vals"])]
        if nd:
            assert subopt_e.dtype == np.float64 and subopt_e.shape == (R,) and subopt_e.flags.c_contiguous
            args.append(p(subopt_e))
        if oa:
            for k in ("oligo_fraction", "bonus"):
                assert state[k].dtype == np.float64 and state[k].shape == (R,) and state[k].flags.c_contiguous
            args += [None] * (not nd) + [p(state["oligo_fraction"]), p(state["bonus"])]
        self._check(getattr(self._L, name + "_oa" if oa else name + "_nd" if nd else name)(*args))

    def mc_run(self, prob, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, flags, rng_state, state,
               counters, best, L_const=504.12, subopt_e=None, self_dimer=False):
        """n_iter Monte-Carlo iterations of all replicas in native code (drna_mc_run).  `state` holds the arrays seqs, mfe_ss
        (uint8 R x L), score, mcc1, Epf, Ed (float64 R); `best` holds seq, ss (uint8 L) and vals (float64 4); all updated in place.
        With `subopt_e` (float64 R, in/out: the second-best energy of every replica's state, kcal/mol) the loop runs the
        negative-design step (drna_mc_run_nd) and `best["vals"]` holds a fifth value, the best state's subopt_e.
        With `self_dimer` (-oa on: drna_mc_run_oa) every proposal is also folded against a copy of itself and
        -kT ln(1 - oligo_fraction) is the last addition to its score; `state` then holds oligo_fraction and bonus (float64 R,
        in/out) and `best["vals"]` has the two-strand layout: 1-MCC, score, Epf, Ed, oligo_fraction, bonus[, subopt_e]."""
        am, partner, snake_of, off, nodes, nst, chars = _packed(prob)
        p = lambda a: a.ctypes.data
        head = [state["seqs"].shape[1], int(n_iter), prob.sec_struct.encode("ascii"), p(partner), p(am), p(snake_of),
                len(prob.snakes), p(off), p(nodes), p(nst), p(chars)]
        self._mc_run("drna_mc_run", head, [int(flags)], ("seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed"), 6 if self_dimer else 4,
                     shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, rng_state, state, counters, best, L_const,
                     subopt_e, oa=bool(self_dimer))

    def mc_run_ragged(self, probs, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, flags, rng_state, state,
                      counters, best, L_const=504.12, R_of=None):
        """:meth:`mc_run` for a set of one-strand ``design.DesignProblem`` s of different lengths, all chains advanced together
        (drna_mc_run_ragged): one ragged scoring call per iteration.  Chains are ordered puzzle after puzzle, puzzle p owning
        ``R_of[p]`` of them (default: ``n_shelves[p]``, a full temperature ladder per puzzle).  `state` holds :meth:`mc_run`'s
        arrays flat: seqs, mfe_ss (uint8, chain after chain), score, mcc1, Epf, Ed (float64 C); shelf_index, temps and rng_state
        have one entry per chain, n_shelves one per puzzle; `counters` is (P, 3); `best` holds seq, ss (uint8, puzzle after
        puzzle) and vals (P, 4).  The call replaces the engine's ragged target set (:meth:`set_targets_ragged`) by the
        puzzles' targets.  Plain ``( ) .`` targets only, no Edef term."""
        self._mc_run_ragged("drna_mc_run_ragged", probs, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f,
                            flags, rng_state, state, counters, best, L_const, R_of, 4, [])

    def mc_run_ragged_nd(self, probs, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, flags, rng_state,
                         state, counters, best, L_const=504.12, R_of=None, subopt_e=None):
        """:meth:`mc_run_ragged` with the auxiliary folds (drna_mc_run_ragged_nd): `scoring_f` may hold an ``Edef`` term (one ragged
        ensemble-defect pass over all chains per iteration), and with `subopt_e` (float64 C, in/out: the second-best energy of every
        chain's state, kcal/mol) the loop runs the negative-design step -- the solved proposals of an iteration, whatever their
        puzzles, in one ragged launch set -- and ``best["vals"]`` is (P, 5), the fifth value the best state's subopt_e."""
        nd = subopt_e is not None
        if nd:
            C_ = int(np.sum(n_shelves if R_of is None else R_of))
            assert subopt_e.dtype == np.float64 and subopt_e.shape == (C_,) and subopt_e.flags.c_contiguous
        self._mc_run_ragged("drna_mc_run_ragged_nd", probs, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f,
                            flags, rng_state, state, counters, best, L_const, R_of, 4 + nd, [subopt_e.ctypes.data if nd else None])

    def _mc_run_ragged(self, name, probs, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, flags, rng_state,
                       state, counters, best, L_const, R_of, n_vals, tail):
        """the call both ragged loops share; `tail`: the arguments behind `best`"""
        P = len(probs)
        ns = np.ascontiguousarray(n_shelves, dtype=np.int32)
        R_of = np.ascontiguousarray(ns if R_of is None else R_of, dtype=np.int32)
        L_of = np.array([p.n for p in probs], dtype=np.int32)
        C_, chars, letters = int(R_of.sum()), int(L_of.sum()), int((R_of.astype(np.int64) * L_of).sum())
        assert ns.shape == (P,) and R_of.shape == (P,)
        _check_rng(rng_state, C_)
        for k in ("seqs", "mfe_ss"):
            assert state[k].dtype == np.uint8 and state[k].shape == (letters,) and state[k].flags.c_contiguous, k
        for k in ("score", "mcc1", "Epf", "Ed"):
            assert state[k].dtype == np.float64 and state[k].shape == (C_,) and state[k].flags.c_contiguous, k
        assert counters.dtype == np.int64 and counters.shape == (P, 3) and counters.flags.c_contiguous
        assert best["vals"].dtype == np.float64 and best["vals"].shape == (P, n_vals) and best["vals"].flags.c_contiguous
        for k in ("seq", "ss"):
            assert best[k].dtype == np.uint8 and best[k].shape == (chars,) and best[k].flags.c_contiguous, k
        ids = np.array([self.TERM_IDS[n] for n, _ in scoring_f], dtype=np.int32)
        ws = np.array([w for _, w in scoring_f], dtype=np.float64)
        sh = np.ascontiguousarray(shelf_index, dtype=np.int32)
        tt = np.ascontiguousarray(temps, dtype=np.float64)
        assert sh.shape == (C_,) and tt.shape == (C_,)
        am = np.concatenate([_packed(q)[0] for q in probs]).astype(np.uint8)
        p = lambda a: a.ctypes.data
        self._check(getattr(self._L, name)(
            self._h, P, p(R_of), p(L_of), int(n_iter), "".join(q.sec_struct for q in probs).encode("ascii"), p(am), p(sh), p(ns),
            float(tm_max), float(tm_min), int(bool(targeted)), p(tt), float(L_const), len(ids), p(ids), p(ws), int(flags), p(rng_state),
            *[p(state[k]) for k in ("seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed")], p(counters), p(best["seq"]), p(best["ss"]),
            p(best["vals"]), *tail))
        self.n_ragged_targets = P

    def mc_run_cofold(self, prob, oligo_state, n_iter, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, rng_state,
                      state, counters, best, L_const=504.12, subopt_e=None):
        """:meth:`mc_run` for a two-strand ``design.DesignProblem`` (drna_mc_run_cofold).  The strings of `state` (seqs, mfe_ss:
        uint8 R x (L + 1)) and of `best` carry the '&'; `state` also holds oligo_fraction and bonus (float64 R), `best["vals"]` six
        values (1-MCC, score, Epf, Ed, oligo_fraction, bonus); set_targets() holds the target without the '&'.  With `subopt_e`
        (float64 R, in/out) the loop runs the negative-design step (drna_mc_run_cofold_nd) and `best["vals"]` holds a seventh
        value, the best state's subopt_e."""
        am = co_allowed_mask(prob)
        head = [state["seqs"].shape[1] - 1, prob.sec_struct.index("&"), int(n_iter), prob.sec_struct.encode("ascii"), am.ctypes.data,
                OLIGO_STATES[oligo_state]]
        self._mc_run("drna_mc_run_cofold", head, [], ("seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed", "oligo_fraction", "bonus"), 6,
                     shelf_index, n_shelves, tm_max, tm_min, targeted, temps, scoring_f, rng_state, state, counters, best, L_const,
                     subopt_e)

    def self_dimer(self, seqs):
        """Every sequence folded against a copy of itself (the reference's ``RNA.fold_compound(s + "&" + s).pf_dimer()`` of -o on,
        utils/energy_scores.py:412-419): dict(FA, FcAA, FAA (kcal/mol, float64[R]; FAA is cofold_batch's FAB of s & s),
        oligo_fraction (dimer_multichain_energy.oligo_fraction)).  The engine needs max_L >= len(s), not twice that; any
        number of sequences."""
        R, L = _equal_length(seqs)
        F4 = np.zeros((R, 4), dtype=np.float64)
        frac = np.zeros(R, dtype=np.float64)
        self._check(self._L.drna_self_dimer_batch(self._h, R, L, "".join(seqs).encode("ascii"), F4.ctypes.data, frac.ctypes.data))
        return {"FA": F4[:, 0], "FcAA": F4[:, 2], "FAA": F4[:, 3], "oligo_fraction": frac}

    def unpaired_free_energy(self, seqs, masks):
        """Free energy (kcal/mol) of every sequence's ensemble with the positions of each mask held unpaired
        (drna_pf_unpaired_batch; RNAfold -p under the hard constraint 'x'): an (R, M) float64 array.  `masks` (see
        :func:`mask_array`) are shared by all sequences; an all-zero mask gives the unconstrained Epf.  Any number of sequences
        and masks."""
        R, L = _equal_length(seqs)
        m = mask_array(masks, L)
        F = np.zeros((R, m.shape[0]), dtype=np.float64)
        self._check(self._L.drna_pf_unpaired_batch(self._h, R, L, "".join(seqs).encode("ascii"), m.shape[0], m.ctypes.data, F.ctypes.data))
        return F

    def opening_energy(self, seqs, masks, Epf=None):
        """(Eopen, p_unpaired), both (R, M): Eopen = F[mask] - Epf (kcal/mol, >= 0 up to rounding) is what it costs to free the
        masked region, p_unpaired = exp(-Eopen / kT) the probability that all of it is unpaired.  `Epf` (R values): the
        sequences' unconstrained ensemble free energies if the caller has them (score_batch's Epf), else they come from one extra
        all-zero mask in the same call."""
        R, L = _equal_length(seqs)
        m = mask_array(masks, L)
        if Epf is None:
            F = self.unpaired_free_energy(seqs, np.concatenate([m, np.zeros((1, L), dtype=np.uint8)]))
            F, F0 = F[:, :-1], F[:, -1]
        else:
            F, F0 = self.unpaired_free_energy(seqs, m), np.asarray(Epf, dtype=np.float64).reshape(R)
        Eopen = F - F0[:, None]
        return Eopen, np.exp(-Eopen / KT)

    def last_access_timing(self):
        """device ms of the last :meth:`unpaired_free_energy` call's launches, summed over its chunks (drna_last_access_timing)"""
        t = C.c_float(0)
        self._check(self._L.drna_last_access_timing(self._h, C.byref(t)))
        return t.value

    def subopt_energy(self, seqs, want_both=False):
        """Energy (dcal/mol) of the second-best structure of each sequence as the reference's -nd on path takes it from
        ViennaRNA's subopt (0 if none within 49 kcal/mol); with want_both also the (R, 2) array of the two lowest energies."""
        R, L = _equal_length(seqs)
        E2 = np.zeros(R, dtype=np.int32)
        E12 = np.zeros((R, 2), dtype=np.int32) if want_both else None
        self._check(self._L.drna_subopt_energy_batch(self._h, R, L, "".join(seqs).encode("ascii"), E2.ctypes.data,
                                                     E12.ctypes.data if want_both else None))
        return (E2, E12) if want_both else E2

    def subopt_energy_ragged(self, seqs, want_both=False):
        """:meth:`subopt_energy` for sequences of DIFFERENT lengths in one call (drna_subopt_energy_ragged): per sequence the
        values of :meth:`subopt_energy` on its own length.  At most ``workspace_slots`` sequences."""
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        R = len(lens)
        E2 = np.zeros(R, dtype=np.int32)
        E12 = np.zeros((R, 2), dtype=np.int32) if want_both else None
        self._check(self._L.drna_subopt_energy_ragged(self._h, R, lens.ctypes.data, "".join(seqs).encode("ascii"), E2.ctypes.data,
                                                      E12.ctypes.data if want_both else None))
        return (E2, E12) if want_both else E2

    def cofold_subopt_energy(self, seqs, want_both=False):
        """Two strands: energy (dcal/mol) of the second-best co-fold structure of each 'AAAA&BBBB' pair as the reference's -nd on
        path takes it from ViennaRNA's subopt on the dimer fold compound (0 if none within 49 kcal/mol); with want_both also
        the (R, 2) array of the two lowest energies (second = 10000000 if there is one structure only)."""
        flat, R, L, cut = _split_pairs(seqs)
        E2 = np.zeros(R, dtype=np.int32)
        E12 = np.zeros((R, 2), dtype=np.int32) if want_both else None
        self._check(self._L.drna_cofold_subopt_energy_batch(self._h, R, L, cut, flat, E2.ctypes.data,
                                                            E12.ctypes.data if want_both else None))
        return (E2, E12) if want_both else E2

    def subopt_structs(self, seqs, K):
        """The K (<= 8) lowest-energy structures of each sequence: (R, K) int32 energies in dcal/mol (ascending; 10000000 where
        a sequence has fewer structures) and a list of R lists of K dot-bracket strings.  Rank k is entry k of ViennaRNA's
        energy-sorted subopt list as get_first_suboptimal_structure_and_energy(seq, fc, k) indexes it (reference
        utils/energy_scores.py:453-488); the order among structures of equal energy is the engine's own."""
        R, L = _equal_length(seqs)
        E = np.zeros((R, K), dtype=np.int32)
        ss = np.zeros((R, K, L), dtype=np.uint8)
        self._check(self._L.drna_subopt_structs_batch(self._h, R, L, "".join(seqs).encode("ascii"), int(K), E.ctypes.data,
                                                      ss.ctypes.data))
        raw = ss.tobytes().decode("ascii")
        return E, [[raw[(r * K + k) * L:(r * K + k + 1) * L] for k in range(K)] for r in range(R)]

    def cofold_subopt_structs(self, seqs, K):
        """Two strands: the K (<= 8) lowest-energy co-fold structures of each 'AAAA&BBBB' pair (equal cut): (R, K) int32 energies
        in dcal/mol (ascending; 10000000 where a pair has fewer structures) and a list of R lists of K dot-bracket strings
        with the '&' put back at the cut.  Rank k is what get_first_suboptimal_structure_and_energy(seq, fc, k) takes from the
        dimer fold compound; the structures and energies are those of :meth:`cofold_batch`'s MFE, the order among structures
        of equal energy is the engine's own."""
        flat, R, L, cut = _split_pairs(seqs)
        E = np.zeros((R, K), dtype=np.int32)
        ss = np.zeros((R, K, L), dtype=np.uint8)
        self._check(self._L.drna_cofold_subopt_structs_batch(self._h, R, L, cut, flat, int(K), E.ctypes.data, ss.ctypes.data))
        raw = ss.tobytes().decode("ascii")
        rows = [[raw[(r * K + k) * L:(r * K + k + 1) * L] for k in range(K)] for r in range(R)]
        return E, [[x[:cut] + "&" + x[cut:] for x in row] for row in rows]

    def ensemble_defect(self, seqs, want_bpp=False):
        """String form of :meth:`ensemble_defect_arrays` (seqs: list of equal-length strings)."""
        return self.ensemble_defect_arrays(_as_u8(seqs), want_bpp)

    def cofold_ensemble_defect(self, seqs, want_bpp=False):
        """Two strands: ensemble defect of each 'AAAA&BBBB' pair against targets[0] ('&' removed) in the ensemble of
        :meth:`cofold_batch`'s partition function (connected structures weighted by expDuplexInit, halved for two equal
        strands).  Returns float64[R]; with want_bpp also the (R, L+1, L+1) pair probabilities over the concatenation
        (1-based, upper triangle)."""
        flat, R, L, cut = _split_pairs(seqs)
        ed = np.zeros(R, dtype=np.float64)
        bpp = np.zeros((R, L + 1, L + 1), dtype=np.float64) if want_bpp else None
        self._check(self._L.drna_cofold_ensemble_defect_batch(self._h, R, L, cut, flat, ed.ctypes.data,
                                                              bpp.ctypes.data if want_bpp else None))
        return (ed, bpp) if want_bpp else ed

    def ensemble_defect_arrays(self, seqs_u8, want_bpp=False):
        """Ensemble defect of each sequence ((R, L) uint8 ASCII letters) against targets[0] (reference
        ScoreSeq.get_ensemble_defect, utils/energy_scores.py:362-374).  Returns float64[R]; with want_bpp also the
        (R, L+1, L+1) base-pair probability matrices (1-based, upper triangle).  R is not limited by max_R.  Sequences of at
        most ``get_option("edef_lds_max")`` nucleotides (pairs: ``"cofold_edef_lds_max"``) take one fused launch with every table
        in LDS (option ``"edef_lds"``, default 1; the counter ``"edef_lds_calls"`` counts those launches)."""
        seqs_u8 = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
        R, L = seqs_u8.shape
        ed = np.zeros(R, dtype=np.float64)
        bpp = np.zeros((R, L + 1, L + 1), dtype=np.float64) if want_bpp else None
        self._check(self._L.drna_ensemble_defect_batch(self._h, R, L, seqs_u8.ctypes.data_as(C.c_char_p), ed.ctypes.data,
                                                       bpp.ctypes.data if want_bpp else None))
        return (ed, bpp) if want_bpp else ed

    def ensemble_defect_device(self, d_seqs, R, L, d_edef, d_bpp=None):
        """Device-resident variant of :meth:`ensemble_defect_arrays` (drna_ensemble_defect_batch_device): raw device pointers to
        the R x L letters, to float64[R] for the defects and, optionally, to the (R, L+1, L+1) matrices, which the caller has
        ZEROED (the outside pass writes the pairs only).  The caller must have made the inputs visible before the call."""
        self._check(self._L.drna_ensemble_defect_batch_device(self._h, int(R), int(L), d_seqs, d_edef, d_bpp))

    def ensemble_defect_ragged(self, seqs, target_of):
        """String form of :meth:`ensemble_defect_ragged_arrays` (seqs: strings of different lengths)."""
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        return self.ensemble_defect_ragged_arrays(np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8), lens, target_of)

    def ensemble_defect_ragged_arrays(self, flat_u8, lens, target_of):
        """Ensemble defect of sequences of DIFFERENT lengths in one call (drna_ensemble_defect_ragged): flat_u8 holds their letters
        back to back (uint8, sum(lens)), target_of[r] names the structure of :meth:`set_targets_ragged` sequence r is measured
        against.  Returns float64[R], per sequence the value of :meth:`ensemble_defect` on its own length and target.  No pair
        probabilities.  All sequences of at most ``get_option("edef_lds_max")`` nucleotides share ONE fused launch."""
        flat_u8 = np.ascontiguousarray(flat_u8, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        tof = np.ascontiguousarray(target_of, dtype=np.int32)
        R = len(lens)
        if flat_u8.shape != (int(lens.sum()),):
            raise ValueError("flat_u8 must hold sum(lens) letters")
        if tof.shape != (R,):
            raise ValueError("target_of must name one structure per sequence")
        ed = np.zeros(R, dtype=np.float64)
        self._check(self._L.drna_ensemble_defect_ragged(self._h, R, lens.ctypes.data, flat_u8.ctypes.data_as(C.c_char_p),
                                                        tof.ctypes.data, ed.ctypes.data))
        return ed

    def sample_structures(self, seqs, S, seed=0):
        """String form of :meth:`sample_structures_arrays`: (R lists of S dot-bracket strings, E (R, S) int32, Epf (R,))."""
        ss, E, Epf = self.sample_structures_arrays(_as_u8(seqs), S, seed)
        R, _, L = ss.shape
        raw = ss.tobytes().decode("ascii")
        return [[raw[(r * S + k) * L:(r * S + k + 1) * L] for k in range(S)] for r in range(R)], E, Epf

    def sample_structures_arrays(self, seqs_u8, S, seed=0):
        """S structures per sequence ((R, L) uint8 ASCII letters) drawn from its Boltzmann ensemble (stochastic traceback on the
        partition function's tables; ViennaRNA's pbacktrack).  Returns (ss (R, S, L) uint8 of ``( ) .``, E (R, S) int32 in
        dcal/mol, Epf (R,) in kcal/mol).  An integer ``seed`` gives sequence r the seed ``seed + r`` (mod 2^64); an array of R
        uint64 gives the seeds themselves.  Sample s of a sequence depends on the sequence, its seed and s alone.
        R is not limited by max_R; ``R * S * L`` is (1 << 30 at most)."""
        seqs_u8 = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
        R, L = seqs_u8.shape
        S = int(S)
        seeds = _sample_seeds(seed, R)
        ss = np.zeros((R, max(S, 0), L), dtype=np.uint8)
        E = np.zeros((R, max(S, 0)), dtype=np.int32)
        Epf = np.zeros(R, dtype=np.float64)
        self._check(self._L.drna_sample_structures_batch(self._h, R, L, seqs_u8.ctypes.data_as(C.c_char_p), S, seeds.ctypes.data,
                                                         ss.ctypes.data, E.ctypes.data, Epf.ctypes.data))
        return ss, E, Epf

    def cofold_sample_structures(self, seqs, S, seed=0):
        """Two strands: S co-fold structures per 'AAAA&BBBB' pair drawn from the ensemble of :meth:`cofold_batch`'s partition
        function (connected structures weighted by expDuplexInit, halved for two equal strands, where a structure and its
        rotation are two structures; the weights sum to exp(-FAB / kT)).  Returns (R lists of S dot-bracket strings with the
        ``&`` put back at the cut, E (R, S) int32 in dcal/mol -- :meth:`cofold_batch`'s E(structure), DuplexInit included for a
        connected structure --, F4 (R, 4): FA, FB, FcAB, FAB in kcal/mol).  Seeds as for :meth:`sample_structures`: an integer
        gives pair r the seed ``seed + r`` (mod 2^64), an array of R uint64 the seeds themselves; sample s of a pair depends on
        the two sequences, its seed and s alone.  R is not limited by max_R."""
        flat, R, L, cut = _split_pairs(seqs)
        S = int(S)
        seeds = _sample_seeds(seed, R)
        ss = np.zeros((R, max(S, 0), L), dtype=np.uint8)
        E = np.zeros((R, max(S, 0)), dtype=np.int32)
        F4 = np.zeros((R, 4), dtype=np.float64)
        self._check(self._L.drna_cofold_sample_structures_batch(self._h, R, L, cut, flat, S, seeds.ctypes.data, ss.ctypes.data,
                                                                E.ctypes.data, F4.ctypes.data))
        raw = ss.tobytes().decode("ascii")
        out = [[raw[(r * S + k) * L:(r * S + k) * L + cut] + "&" + raw[(r * S + k) * L + cut:(r * S + k + 1) * L] for k in range(S)]
               for r in range(R)]
        return out, E, F4

    def _mea(self, flat, R, L, cut, gamma, want_bpp):
        mea = np.zeros((R, L), dtype=np.uint8)
        cen = np.zeros((R, L), dtype=np.uint8)
        val = np.zeros(R, dtype=np.float64)
        dist = np.zeros(R, dtype=np.float64)
        E = np.zeros((R, 2), dtype=np.int32)
        bpp = np.zeros((R, L + 1, L + 1), dtype=np.float64) if want_bpp else None
        tail = (float(gamma), mea.ctypes.data, val.ctypes.data, cen.ctypes.data, dist.ctypes.data, E.ctypes.data,
                bpp.ctypes.data if want_bpp else None)
        if cut:
            self._check(self._L.drna_cofold_mea_structures_batch(self._h, R, L, cut, flat, *tail))
        else:
            self._check(self._L.drna_mea_structures_batch(self._h, R, L, flat, *tail))
        put = (lambda x: x[:cut] + "&" + x[cut:]) if cut else (lambda x: x)
        txt = lambda a: [put(row.tobytes().decode("ascii")) for row in a]
        out = {"mea": txt(mea), "mea_value": val, "centroid": txt(cen), "centroid_distance": dist, "E": E}
        if want_bpp:
            out["bpp"] = bpp
        return out

    def mea_structures(self, seqs, gamma=1.0, want_bpp=False):
        """The two structures that represent each sequence's ensemble, read from its pair probabilities on the device
        (ViennaRNA's fc.MEA(gamma) and fc.centroid(); drna_mea_structures_batch).  Returns a dict: ``mea`` (R dot-bracket
        strings, a maximiser of the expected accuracy sum_unpaired q(i) + 2 gamma sum_pairs P(i,j)), ``mea_value`` (R,),
        ``centroid`` (the pairs with P > 1/2), ``centroid_distance`` (R,; its expected base-pair distance to the ensemble),
        ``E`` ((R, 2) int32, dcal/mol: MEA, centroid) and, with want_bpp, ``bpp`` ((R, L+1, L+1), the matrix of
        :meth:`ensemble_defect`).  Needs no targets and leaves installed ones alone; R is not limited by max_R."""
        u8 = np.ascontiguousarray(_as_u8(seqs), dtype=np.uint8)
        R, L = u8.shape
        return self._mea(u8.ctypes.data_as(C.c_char_p), R, L, 0, gamma, want_bpp)

    def cofold_mea_structures(self, seqs, gamma=1.0, want_bpp=False):
        """Two strands: :meth:`mea_structures` of each 'AAAA&BBBB' pair in the ensemble of :meth:`cofold_ensemble_defect`
        (drna_cofold_mea_structures_batch).  The strings carry the ``&`` at the cut; ``E`` is :meth:`cofold_batch`'s
        E(structure), DuplexInit included for a connected structure; ``bpp`` is over the concatenation."""
        flat, R, L, cut = _split_pairs(seqs)
        return self._mea(flat, R, L, cut, gamma, want_bpp)

    def last_mea_timing(self):
        """device ms of the last :meth:`mea_structures` / :meth:`cofold_mea_structures` call, summed over its chunks"""
        out = (C.c_float * 3)()
        self._check(self._L.drna_last_mea_timing(self._h, out))
        return {"inside": out[0], "outside": out[1], "mea": out[2]}

    def last_edef_timing(self):
        out = (C.c_float * 2)()
        self._check(self._L.drna_last_edef_timing(self._h, out))
        return {"inside": out[0], "outside": out[1]}

    def last_timing(self):
        """ms of device time of the last call: dict(mfe, pf, eval, total) from HIP events on the engine's streams."""
        out = (C.c_float * 4)()
        self._check(self._L.drna_last_timing(self._h, out))
        return {"mfe": out[0], "pf": out[1], "eval": out[2], "total": out[3]}

    def timing_sums(self, reset=False):
        """device ms summed over the score_batch[_device] calls since the last reset: dict(mfe, pf, eval, total, calls)"""
        out = (C.c_double * 5)()
        self._check(self._L.drna_timing_sums(self._h, out, int(bool(reset))))
        return {"mfe": out[0], "pf": out[1], "eval": out[2], "total": out[3], "calls": int(out[4])}

    def info(self):
        out = (C.c_int64 * 6)()
        self._check(self._L.drna_info(self._h, out))
        return {"device": out[0], "max_R": out[1], "max_L": out[2], "threads_per_wg": out[3],
                "compute_units": out[4], "workspace_bytes": out[5]}


class HostKernels:
    """Native batched host helpers of the MC inner loop (no GPU needed): SimScore, proposals, Metropolis, the motif term."""

    def __init__(self, lib=None):
        self._L = load_library(lib)

    @staticmethod
    def _pack(prob):
        """arrays of a design.DesignProblem in the layout of drna_propose_batch_alt / drna_mc_run (cached on the problem)"""
        am = co_allowed_mask(prob)
        partner = np.ascontiguousarray(prob.partner, dtype=np.int32)
        snake_of = np.ascontiguousarray(prob.snake_of, dtype=np.int32)
        off, nodes, nst, chars = [0], [], [], b""
        for nd, states in prob.snakes:
            nodes += list(nd)
            off.append(len(nodes))
            nst.append(len(states))
            chars += "".join(states).encode() + b"." * (len(nd) * (4 - len(states)))
        prob._native_pack = (am, partner, snake_of, np.array(off, dtype=np.int32), np.array(nodes or [0], dtype=np.int32),
                             np.array(nst or [0], dtype=np.int32), np.frombuffer(chars or b".", dtype=np.uint8).copy())

    def rng_seed(self, seeds, out=None):
        """One MT19937 stream per entry of `seeds`, seeded like ``random.seed(int)`` (the reference re-seeds every worker
        with its replica index at each exchange step, utils/replica_exchange_monte_carlo.py:227-228,250)."""
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        st = out if out is not None else np.empty((sd.shape[0], RNG_WORDS), dtype=np.uint32)
        assert st.dtype == np.uint32 and st.shape == (sd.shape[0], RNG_WORDS) and st.flags.c_contiguous
        rc = self._L.drna_rng_seed(sd.shape[0], sd.ctypes.data, st.ctypes.data)
        if rc != 0:
            raise EngineError(rc, "drna_rng_seed")
        return st

    def rng_random(self, rng_state):
        """one ``random.random()`` from every stream"""
        out = np.empty(rng_state.shape[0])
        rc = self._L.drna_rng_random(rng_state.shape[0], rng_state.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise EngineError(rc, "drna_rng_random")
        return out

    def simscore(self, ref, queries_u8):
        """ref: reference structure string ('&' -> 'Ee' already applied); queries_u8: (R, L) uint8.
        Returns rounded (mcc, recall, precision) arrays exactly as the reference's SimScore computes them."""
        q = np.ascontiguousarray(queries_u8, dtype=np.uint8)
        R, L = q.shape
        mcc, rec, prec = np.zeros(R), np.zeros(R), np.zeros(R)
        rc = self._L.drna_simscore_batch(R, L, ref.encode("ascii"), q.ctypes.data, mcc.ctypes.data, rec.ctypes.data,
                                         prec.ctypes.data)
        if rc != 0:
            raise EngineError(rc, "drna_simscore_batch")
        return mcc, rec, prec

    def motif_score(self, motifs, seqs_u8):
        """The motif term of every sequence of seqs_u8 ((R, L) uint8; two strands with the '&' column): 0 + the values of the
        motifs that occur in it, in their order (drna_motif_score_batch).  `motifs` as for ``Engine.set_motifs``."""
        s = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
        R, L = s.shape
        n, lens, keys, values = _motif_arrays(motifs)
        out = np.zeros(R, dtype=np.float64)
        rc = self._L.drna_motif_score_batch(R, L, s.ctypes.data, n, lens.ctypes.data, keys, values.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise EngineError(rc, "drna_motif_score_batch")
        return out

    def _propose(self, name, struct, problem, seqs_u8, ss_u8, shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state):
        """drna_propose_batch[_alt|_co] (`name`): `problem` are the arguments between the structure and the sequences"""
        s = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
        R, L = s.shape
        out = np.empty_like(s)
        ss = np.ascontiguousarray(ss_u8, dtype=np.uint8)
        sh = np.ascontiguousarray(shelf_index, dtype=np.int32)
        _check_rng(rng_state, R)
        rc = getattr(self._L, name)(R, L, struct.encode("ascii"), *problem, s.ctypes.data, ss.ctypes.data, sh.ctypes.data,
                                    int(n_shelves), float(tm_max), float(tm_min), int(bool(targeted)), rng_state.ctypes.data,
                                    out.ctypes.data)
        if rc != 0:
            raise EngineError(rc, name)
        return out

    def propose(self, target, allowed_mask, seqs_u8, ss_u8, shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state):
        am = np.ascontiguousarray(allowed_mask, dtype=np.uint8)
        return self._propose("drna_propose_batch", target, [am.ctypes.data], seqs_u8, ss_u8, shelf_index, n_shelves, tm_max, tm_min,
                             targeted, rng_state)

    def propose_alt(self, prob, seqs_u8, ss_u8, shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state):
        """Proposals for a ``design.DesignProblem`` that may hold alternative-structure snakes."""
        am, partner, snake_of, off, nodes, nst, chars = _packed(prob)
        problem = [partner.ctypes.data, am.ctypes.data, snake_of.ctypes.data, len(prob.snakes), off.ctypes.data, nodes.ctypes.data,
                   nst.ctypes.data, chars.ctypes.data]
        return self._propose("drna_propose_batch_alt", prob.sec_struct, problem, seqs_u8, ss_u8, shelf_index, n_shelves, tm_max,
                             tm_min, targeted, rng_state)

    def propose_co(self, prob, oligo_state, seqs_u8, ss_u8, shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state):
        """Proposals for a two-strand ``design.DesignProblem`` (drna_propose_batch_co): the strings keep the '&';
        oligo_state "heterodimer" or "homodimer" (the reference's strand-copy rules follow every move)."""
        am = co_allowed_mask(prob)
        return self._propose("drna_propose_batch_co", prob.sec_struct, [am.ctypes.data, OLIGO_STATES[oligo_state]], seqs_u8, ss_u8,
                             shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state)

    def metropolis(self, score_o, score_m, temps, rng_state, L_const=504.12):
        so = np.ascontiguousarray(score_o, dtype=np.float64)
        sm = np.ascontiguousarray(score_m, dtype=np.float64)
        tt = np.ascontiguousarray(temps, dtype=np.float64)
        R = so.shape[0]
        _check_rng(rng_state, R)
        acc = np.zeros(R, dtype=np.uint8)
        bet = np.zeros(R, dtype=np.uint8)
        rc = self._L.drna_metropolis_batch(R, so.ctypes.data, sm.ctypes.data, tt.ctypes.data, float(L_const),
                                           rng_state.ctypes.data, acc.ctypes.data, bet.ctypes.data)
        if rc != 0:
            raise EngineError(rc, "drna_metropolis_batch")
        return acc.astype(bool), bet.astype(bool)
