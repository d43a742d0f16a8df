"""Scoring function of the design loop, batched over replicas and backed by the gfx950 engine.

Counterpart of the reference's ``utils/energy_scores.py``: ``score_sequence`` (:31-125),
``get_mfe_e_ss`` (:128-159) and ``ScoreSeq`` (:162-450).  The ``-sf`` plug-in surface is unchanged:
the same term names (``Ed-Epf``, ``1-MCC``, ``sln_Epf``, ``Ed-MFE``, ``1-precision``, ``1-recall``,
``Edef``) with the same weights and x10 factors (:376-398), the alt-structure term (:98-102) and the
motif bonus (:121-123, :443-450).  What changes is where the numbers come from: one engine call returns
Epf, the MFE (or pk-annotated) structure, the MFE energy and E(target), E(alt targets) for every replica
of the batch, instead of 3-8 ViennaRNA calls per sequence inside a forked worker.

There is ONE scorer and it works on arrays: ``SF_TERMS`` is the ``-sf`` table (name, native id, formula),
:func:`score_arrays` scores an (R, L) uint8 batch of candidates -- one strand, two strands, alternative structures,
``-nd on`` -- in the reference's order of additions, and :func:`record` turns one row of its result into a ``ScoreSeq``.
``ReplicaScorer.score`` (``design.run_design``) is ``record`` over every row, plus ``-oa`` (through its own 2 L engine;
``score_arrays(self_dimer=True)`` is the fast driver's form, ``Engine.self_dimer``) and the motifs (``score_motifs`` on the
regular expressions of :func:`parse_motifs`; ``score_arrays(motifs=...)`` is the fast drivers' form, ``HostKernels.motif_score``);
``design.run_design_fast`` keeps the arrays as its replica state and calls ``record`` for its records only.  The native
loop (``mc_loop`` in ``csrc/engine.hip``) is the same sum in C, on the same term ids.

``Edef`` is served by ``Engine.ensemble_defect_arrays`` (inside + outside recursion on the GPU), for two strands by
``Engine.cofold_ensemble_defect`` (the outside recursion under the co-fold rules; no golden in the reference: checked against
exhaustive enumeration); two-strand ``Ed-MFE`` takes the co-fold MFE energy.

Two strands (``oligo_state`` heterodimer / homodimer, and ``avoid`` = ``-o on``) go through ``Engine.cofold_batch``
(co-fold MFE + partition function + two-strand evaluation on the GPU); the oligomer / monomer bonus terms of
``utils/dimer_multichain_energy.py`` are computed here from its free energies.

``-nd on`` (negative design): the energy of the second-best structure comes from ``Engine.subopt_energy`` (two-best
dynamic programme on the GPU; no golden in the reference: checked against exhaustive enumeration), for two strands from
``Engine.cofold_subopt_energy`` (the same programme under the co-fold rules).
"""
from types import SimpleNamespace

import numpy as np

from . import engine as _engine

# reference utils/dimer_multichain_energy.py:24-28
KB = 0.001987204259
RHO = 55.14
TEMP = 273.15 + 37
CONC = 1e-3


def oligo_fraction(FA, FB, FcAB):
    """reference dimer_multichain_energy.oligo_fraction (:30-45): fraction of strands bound in the dimer at 1 mM."""
    dF = FcAB - FA - FB
    rhs = CONC / RHO * np.exp(-dF / (KB * TEMP))
    return 1 - (np.sqrt(1 + 4 * rhs) - 1) / (2 * rhs)


def kTlog_oligo_fraction(frac):
    return -KB * TEMP * np.log(frac)


def kTlog_monomer_fraction(frac):
    return -KB * TEMP * np.log(1 - frac)


# THE -sf table (reference :376-398): name, native id (the case mc_loop switches on, = Engine.TERM_IDS), and the term's value from
# v.Epf, v.Ed = E(target), v.Emfe (kcal/mol), the rounded v.mcc1 = 1 - MCC, v.recall1, v.precision1, the ensemble defect v.Edef and
# the string length v.n (two strands: with the '&'): a batch's arrays (score_arrays) or one record's numbers (ScoreSeq)
SF_TERMS = (("Ed-Epf", 0, lambda v: v.Ed - v.Epf), ("1-MCC", 1, lambda v: v.mcc1 * 10),
            ("sln_Epf", 2, lambda v: (v.Epf + 0.3759 * v.n + 5.7534) / 10), ("Ed-MFE", 3, lambda v: v.Ed - v.Emfe),
            ("1-precision", 4, lambda v: v.precision1 * 10), ("1-recall", 5, lambda v: v.recall1 * 10),
            ("Edef", 6, lambda v: v.Edef))
AVAILABLE_SCORING_FUNCTIONS = [name for name, _, _ in SF_TERMS]
_TERM = {name: value for name, _, value in SF_TERMS}


def check_scoring_functions(scoring_f):
    for function, _ in scoring_f:
        if function not in _TERM:
            raise ValueError("%s is not an available option for scoring function. Check your command." % function)


def sf_sum(scoring_f, v):
    """the -sf sum, from 0, in -sf order, of the values `v` (see SF_TERMS); a name that is not in the table adds nothing, as in
    the reference"""
    total = 0
    for function, weight in scoring_f:
        if function in _TERM:
            total += _TERM[function](v) * weight
    return total


def parse_scoring_functions(scoring_f_str, first_term_only=True):
    """``-sf`` string -> [(name, weight), ...].

    ``first_term_only=True`` reproduces the reference, whose ``return`` sits inside the loop
    (``utils/stats_inputs_outputs.py:232-237``): only the first term survives.
    """
    out = []
    for item in scoring_f_str.split(','):
        if ':' not in item:
            raise ValueError(f"Invalid scoring function format: {item}. Expected format: 'function:weight'")
        function, weight = item.split(':')
        out.append((function, float(weight)))
        if first_term_only:
            return out
    return out


class ScoreSeq:
    """Per-replica state record.  The attribute NAMES and their ORDER are the reference's (``vars(obj)`` is its CSV schema,
    ``utils/energy_scores.py:176-195``) and so are the method names the host code calls; the setters themselves are generated
    from three small tables below the class instead of being written out one by one."""

    # (attribute, initial value) in the order of the reference's __init__ = the column order of _traj.csv / _results.csv
    _SCHEMA = (("sequence", None), ("scoring_function", 0), ("replica_num", None), ("temp_shelf", None), ("sim_step", 0),
               ("edesired_minus_Epf", 0), ("Epf", 0), ("edesired", 0), ("mcc", 0), ("mcc_alt", 0), ("mfe_ss", None),
               ("subopt_e", 0), ("esubopt_minus_Epf", 0), ("sln_Epf", 0), ("MFE", 0), ("edesired_minus_MFE", 0), ("recall", 0),
               ("precision", 0), ("edesired2", 0), ("edesired2_minus_Epf", 0))
    def __init__(self, sequence):
        for name, value in self._SCHEMA:
            setattr(self, name, value)
        self.sequence = sequence

    def get_sln_Epf(self):
        self.sln_Epf = (self.Epf + 0.3759 * len(self.sequence) + 5.7534) / 10

    def get_edesired_minus_MFE(self):
        self.edesired_minus_MFE = self.edesired - self.MFE

    def get_scoring_function_w_subopt(self):
        self.scoring_function = self.scoring_function - self.esubopt_minus_Epf

    def get_scoring_function(self, scoring_f):
        self.scoring_function = sf_sum(scoring_f, SimpleNamespace(
            Epf=self.Epf, Ed=self.edesired, Emfe=self.MFE, mcc1=self.mcc, recall1=self.recall, precision1=self.precision,
            Edef=getattr(self, "ensemble_defect", None), n=len(self.sequence)))

    def get_scoring_function_w_alt_ss(self):
        self.scoring_function = self.scoring_function + self.edesired2_minus_Epf

    def update_scoring_function_w_motifs(self, motif_bonus):
        self.scoring_function += motif_bonus


def _install_setters(cls):
    """``get_<attr>(value)`` stores a value as it comes (MFE: the reference re-folds with RNA.fold(), :350-354, the engine's fill
    already produced f5[n]; ensemble_defect: the reference runs mfe / rescale / pf / ensemble_defect on a new fold compound,
    :362-374, here the value comes from the engine's inside + outside kernels -- and the attribute is created on first use, as
    there); ``get_<attr>(x)`` for precision / recall / mcc stores 1 - x; ``get_<attr>_minus_Epf(Epf, e)`` stores e - Epf."""
    def plain(attr):
        def setter(self, value):
            setattr(self, attr, value)
        return setter

    def complement(attr):
        def setter(self, value):
            setattr(self, attr, 1 - value)
        return setter

    def minus_epf(attr):
        def setter(self, Epf, energy):
            setattr(self, attr, energy - Epf)
        return setter

    for attr in ("replica_num", "temp_shelf", "sim_step", "Epf", "mfe_ss", "edesired", "edesired2", "MFE", "subopt_e", "ensemble_defect"):
        setattr(cls, "get_" + attr, plain(attr))
    for attr in ("precision", "recall", "mcc"):
        setattr(cls, "get_" + attr, complement(attr))
    for attr in ("edesired_minus_Epf", "edesired2_minus_Epf", "esubopt_minus_Epf"):
        setattr(cls, "get_" + attr, minus_epf(attr))


_install_setters(ScoreSeq)


# letters of a -motifs key and the sequence letters each stands for (T is a letter of its own: N does not match it)
MOTIF_LETTERS = {"A": "A", "C": "C", "G": "G", "U": "U", "T": "T", "W": "AU", "S": "CG", "M": "AC", "K": "GU", "R": "AG", "Y": "CU",
                 "B": "CGU", "D": "AGU", "H": "ACU", "V": "ACG", "N": "ACGU"}


def parse_motifs(text):
    """``-motifs KEY,VALUE,KEY,VALUE,...`` (reference DesiRNA.py:212-224) -> the dict ``sim_options.motifs`` holds there:
    key -> (compiled regular expression, float value), in the order given; a repeated key keeps its first position and takes
    its last value; the empty key is legal and occurs in every sequence.  An empty text: no motifs.  An odd number of items, a
    letter outside ``MOTIF_LETTERS`` (lower case included) or a value that is no float raises ValueError with the
    reference's message."""
    import re
    if not text:
        return {}
    items = text.split(",")
    try:
        if len(items) % 2:
            raise IndexError(len(items))
        return {key: (re.compile("".join(MOTIF_LETTERS[ch] if len(MOTIF_LETTERS[ch]) == 1 else "[%s]" % MOTIF_LETTERS[ch] for ch in key)),
                      float(value)) for key, value in zip(items[::2], items[1::2])}
    except (KeyError, ValueError, IndexError):
        raise ValueError("Something is wrong with your motifs") from None


def score_motifs(seq, sim_options):
    """reference utils/sequence_utils.py:1231-1251"""
    motif_score = 0
    for motif in sim_options.motifs:
        if sim_options.motifs[motif][0].search(seq):
            motif_score += sim_options.motifs[motif][1]
    return motif_score


def opening_term(eng, seqs, Epf, accessible):
    """(opening_energy, p_unpaired), float64[R]: what it costs every sequence's ensemble to keep the region `accessible` (one
    mask of ``Engine.unpaired_free_energy``: an ``x`` / ``.`` line or a (1, L) array) unpaired, Eopen = F[region unpaired] - Epf
    with the batch's own Epf, and exp(-Eopen / kT), the probability that the whole region is free.  ONE engine call, M = 1"""
    F = eng.unpaired_free_energy(seqs, accessible)
    Eopen = F[:, 0] - np.asarray(Epf, dtype=np.float64)
    return Eopen, np.exp(-Eopen / (KB * TEMP))


def score_arrays(eng, hk, sec_struct, scoring_f, seqs_u8, oligo_state="none", pks="off", nd=False, self_dimer=False, motifs=None,
                 accessible=None, accessible_weight=1.0):
    """THE scorer (reference score_sequence(), :70-118, for a whole batch): `eng` an ``engine.Engine`` whose targets are
    sec_struct (+ the alternative structures) without the '&', `hk` an ``engine.HostKernels``, seqs_u8 the (R, L) uint8 candidates
    (two strands -- oligo_state heterodimer / homodimer --: with the '&' column).  Returns the batch as arrays, named like the
    state of ``Engine.mc_run``: seqs, mfe_ss (uint8 R x L), score, mcc1, recall1, precision1, Epf (two strands: FAB), Ed, and where
    they apply (else None) sln_Epf, Emfe (``-sf Ed-MFE``; kcal/mol), Edef, Ed2 (mean E(alternative structures)), subopt_e (`nd`;
    0 where 1 - MCC != 0), oligo_fraction, bonus (two strands; one strand with `self_dimer`).

    `self_dimer` (opt-in, with oligo_state "avoid" = -oa on only): oligo_fraction of every candidate folded against a copy of
    itself from ``eng.self_dimer`` and bonus = -kT ln(1 - oligo_fraction), added last (reference :118-119, :412-419).  Off by
    default: ``ReplicaScorer.score`` adds that term itself.

    `motifs` (opt-in; :func:`parse_motifs`'s dict, or any form ``HostKernels.motif_score`` takes): the motif term of every
    candidate's string (two strands: with the '&'), the last addition of all (reference :121-123).  Off by default:
    ``ReplicaScorer.score`` adds that term itself, too.

    `accessible` (opt-in, one strand; the ``>accessible`` region of the input as a mask of ``Engine.unpaired_free_energy``):
    :func:`opening_term` of every candidate from one engine call; `accessible_weight` x opening_energy is the last addition of
    all, after the motif term, and the batch carries opening_energy and p_unpaired.  Off by default, and
    ``ReplicaScorer.score`` adds that term itself, after its own motif term.

    The reference's order of additions: the -sf sum; + (Ed2 - Epf) with alternative structures, every energy / 100 first, then
    the sum, then / count (one strand only, as the two-strand scorer always had it); - (subopt_e - Epf) on the candidates with
    1 - MCC == 0 (`nd`: ONE second-best call for that subset); + the oligomer bonus (hetero-dimer, or homodimer with two different
    structures) or the monomer-fraction term (two equal structures)."""
    names = [function for function, _ in scoring_f]
    two = oligo_state in ("heterodimer", "homodimer")
    seqs_u8 = np.ascontiguousarray(seqs_u8, dtype=np.uint8)
    R, L = seqs_u8.shape
    strings = lambda rows: [bytes(seqs_u8[k]).decode() for k in rows]
    b = SimpleNamespace(seqs=seqs_u8, n=L, sln_Epf=None, Emfe=None, Edef=None, Ed2=None, subopt_e=None, oligo_fraction=None, bonus=None)
    if accessible is not None and two:
        raise ValueError("an accessible region takes one strand")
    ref = sec_struct.replace("&", "Ee")
    if two:
        seqs = strings(range(R))
        out = eng.cofold_batch(seqs, _engine.NEED_PF | _engine.NEED_MFE | _engine.NEED_EVAL)
        b.mfe_ss = np.frombuffer("".join(out["mfe_ss"]).encode(), dtype=np.uint8).reshape(R, L).copy()
        cut = sec_struct.index("&")                       # SimScore on the reference's '&' -> 'Ee' substitution
        Ee = np.broadcast_to(np.frombuffer(b"Ee", dtype=np.uint8), (R, 2))
        mcc, rec, prec = hk.simscore(ref, np.concatenate([b.mfe_ss[:, :cut], Ee, b.mfe_ss[:, cut + 1:]], axis=1))
        b.Epf, Emfe, Ed = np.array(out["FAB"], dtype=np.float64), out["Emfe"], out["Ed"][:, :1]
    else:
        flags = _engine.NEED_PF | _engine.NEED_MFE | _engine.NEED_EVAL | (_engine.NEED_PK if pks == "on" else 0)
        b.Epf, Emfe, b.mfe_ss, Ed = eng.score_batch_arrays(seqs_u8, flags)
        mcc, rec, prec = hk.simscore(ref, b.mfe_ss)
    b.mcc1, b.recall1, b.precision1 = 1 - mcc, 1 - rec, 1 - prec
    b.Ed = Ed[:, 0] / 100.0
    if "Ed-MFE" in names:
        b.Emfe = Emfe / 100.0
    if "Edef" in names:                                   # reference :93-94
        b.Edef = eng.cofold_ensemble_defect(seqs) if two else eng.ensemble_defect_arrays(seqs_u8)
    if "sln_Epf" in names:
        b.sln_Epf = _TERM["sln_Epf"](b)
    b.score = np.zeros(R) + sf_sum(scoring_f, b)
    if Ed.shape[1] > 1:                                   # reference :98-102
        total = 0
        for t in range(1, Ed.shape[1]):
            total = total + Ed[:, t] / 100.0
        b.Ed2 = total / (Ed.shape[1] - 1)
        b.score = b.score + (b.Ed2 - b.Epf)
    if nd:                                                # reference :104-108
        b.subopt_e = np.zeros(R)
        hit = np.nonzero(b.mcc1 == 0)[0]
        if len(hit):
            b.subopt_e[hit] = (eng.cofold_subopt_energy if two else eng.subopt_energy)(strings(hit)) / 100.0
            b.score[hit] -= b.subopt_e[hit] - b.Epf[hit]
    if two:                                               # reference :109-116, utils/dimer_multichain_energy.py
        ss1, ss2 = sec_struct.split("&")
        kTlog = kTlog_oligo_fraction if oligo_state == "heterodimer" or ss1 != ss2 else kTlog_monomer_fraction
        b.oligo_fraction = np.array([float(oligo_fraction(out["FA"][k], out["FB"][k], out["FcAB"][k])) for k in range(R)])
        b.bonus = np.array([float(kTlog(f)) for f in b.oligo_fraction])
        b.score = b.score + b.bonus
    elif self_dimer and oligo_state == "avoid":           # reference :118-119, get_scoring_function_monomer (:412-419)
        b.oligo_fraction = np.array(eng.self_dimer(strings(range(R)))["oligo_fraction"], dtype=np.float64)
        b.bonus = np.array([float(kTlog_monomer_fraction(f)) for f in b.oligo_fraction])
        b.bonus_field = "monomer_bonus"
        b.score = b.score + b.bonus
    if motifs:                                            # reference :121-123
        b.score = b.score + hk.motif_score(motifs, seqs_u8)
    if accessible is not None:
        b.opening_energy, b.p_unpaired = opening_term(eng, strings(range(R)), b.Epf, accessible)
        b.score = b.score + accessible_weight * b.opening_energy
    return b


def record(b, k):
    """Row k of a batch of :func:`score_arrays` (or of the arrays ``design.run_design_fast`` keeps of it: what is not there
    stays at the ScoreSeq default) -> ScoreSeq"""
    col = lambda name: None if getattr(b, name, None) is None else float(getattr(b, name)[k])
    sc = ScoreSeq(sequence=bytes(b.seqs[k]).decode())
    sc.scoring_function = col("score")
    sc.get_Epf(col("Epf"))
    sc.get_mfe_ss(bytes(b.mfe_ss[k]).decode())
    sc.get_edesired(col("Ed"))
    sc.get_edesired_minus_Epf(sc.Epf, sc.edesired)
    sc.mcc = col("mcc1")
    if col("recall1") is not None:
        sc.recall, sc.precision = col("recall1"), col("precision1")
    if col("sln_Epf") is not None:
        sc.get_sln_Epf()
    if col("Emfe") is not None:
        sc.get_MFE(col("Emfe"))
        sc.get_edesired_minus_MFE()
    if col("Edef") is not None:
        sc.get_ensemble_defect(col("Edef"))
    if col("Ed2") is not None:
        sc.get_edesired2(col("Ed2"))
        sc.get_edesired2_minus_Epf(sc.Epf, sc.edesired2)
    if col("subopt_e") is not None and sc.mcc == 0:
        sc.get_subopt_e(col("subopt_e"))
        sc.get_esubopt_minus_Epf(sc.Epf, sc.subopt_e)
    if col("oligo_fraction") is not None:
        sc.oligo_fraction = col("oligo_fraction")
        setattr(sc, getattr(b, "bonus_field", "oligomer_bonus"), col("bonus"))     # (-oa on: monomer_bonus, as ReplicaScorer.score names it)
    if col("opening_energy") is not None:
        sc.opening_energy, sc.p_unpaired = col("opening_energy"), col("p_unpaired")
    return sc


class ReplicaScorer:
    """Binds an engine to one design problem (target + alt structures + options) and scores batches: :func:`score_arrays` and
    :func:`record`, plus the two terms ``design.run_design`` adds record by record (-oa on and the motifs)."""

    def __init__(self, input_file, sim_options, max_replicas, device=0, engine=None):
        self.oligo_state = getattr(sim_options, "oligo_state", "none")
        if self.oligo_state not in ("none", "avoid", "heterodimer", "homodimer"):
            raise ValueError("unknown oligo_state %r" % self.oligo_state)
        self.subopt = getattr(sim_options, "subopt", "off") == "on"
        self.input_file = input_file
        self.sim_options = sim_options
        self.target = input_file.sec_struct.replace("&", "")
        L = len(self.target)
        self.engine = engine or _engine.Engine(max_R=max_replicas, max_L=L, device=device,
                                               params=str(getattr(sim_options, "param", "1999")))
        self.hk = _engine.HostKernels()
        # -oa on folds every candidate against itself (s & s: 2 L nucleotides, reference :411-418): that needs an engine
        # sized for 2 L; the scoring engine stays sized for L (its workspace pitch follows max_L)
        self.dimer_engine = self.engine
        if self.oligo_state == "avoid" and self.engine.max_L < 2 * L:
            self.dimer_engine = _engine.Engine(max_R=max(max_replicas, 1), max_L=2 * L, device=device,
                                               params=str(getattr(sim_options, "param", "1999")))
        targets = [self.target]
        if getattr(input_file, "alt_sec_struct", None) is not None:
            targets += [a.replace("&", "") for a in input_file.alt_sec_structs]
        self.engine.set_targets(targets)
        check_scoring_functions(sim_options.scoring_f)

    def score(self, seqs):
        """list of sequences -> list of ScoreSeq (reference score_sequence(), once per replica)."""
        seqs = list(seqs)
        b = score_arrays(self.engine, self.hk, self.input_file.sec_struct, self.sim_options.scoring_f,
                         np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1), self.oligo_state,
                         getattr(self.sim_options, "pks", "off"), self.subopt)
        res = [record(b, k) for k in range(len(seqs))]
        if self.oligo_state == "avoid":
            # reference get_scoring_function_monomer (:411-418): homodimer of the sequence with itself, monomer fraction bonus
            # (applied before the motif bonus in the reference; both are additive)
            co = self.dimer_engine.cofold_batch([s + "&" + s for s in seqs], _engine.NEED_PF)
            for k, sc in enumerate(res):
                sc.oligo_fraction = float(oligo_fraction(co["FA"][k], co["FB"][k], co["FcAB"][k]))
                sc.monomer_bonus = float(kTlog_monomer_fraction(sc.oligo_fraction))
                sc.scoring_function = sc.scoring_function + sc.monomer_bonus
        if getattr(self.sim_options, "motifs", None):
            for seq, sc in zip(seqs, res):
                sc.update_scoring_function_w_motifs(score_motifs(seq, self.sim_options))
        region = getattr(self.sim_options, "accessible", None)
        if region is not None:                                # the last addition of all
            if self.oligo_state in ("heterodimer", "homodimer"):
                raise ValueError("an accessible region takes one strand")
            Eopen, p = opening_term(self.engine, seqs, b.Epf, region)
            w = getattr(self.sim_options, "accessible_weight", 1.0)
            for k, sc in enumerate(res):
                sc.opening_energy, sc.p_unpaired = float(Eopen[k]), float(p[k])
                sc.scoring_function = sc.scoring_function + w * sc.opening_energy
        return res


def score_sequence(seq, input_file, sim_options, scorer=None):
    """Single-sequence form with the reference's signature (a batch of one)."""
    scorer = scorer or ReplicaScorer(input_file, sim_options, max_replicas=1)
    return scorer.score([seq])[0]
