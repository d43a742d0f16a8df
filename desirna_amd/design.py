"""Batched replica-exchange Monte-Carlo design driver on top of the GPU scoring engine.

Counterpart of the reference's host loop: ``run_functions`` (``DesiRNA.py:333-386``),
``mutate_sequence_re`` / ``single_replica_design`` (``utils/replica_exchange_monte_carlo.py:176-271``),
``mutate_sequence`` / ``get_mutation_position`` / ``expand_cases`` (``utils/sequence_utils.py:926-1136``),
``get_nt_list`` (:454-525), ``initial_sequence_generator`` (:686-763) and ``read_input``
(``utils/stats_inputs_outputs.py:183-214``).  SURVEY rows a1, a2, a5 (8(f)-1).

What is kept from the reference: the input-file format, IUPAC sequence restraints, the move set (single
unpaired position / Watson-Crick-or-GU pair move on target pairs), targeted mutations around false
negatives / false positives of the current MFE structure (+-3 window, per-temperature probability
``linspace(tm_max, tm_min, R)`` rounded to 2 dp), the initial-sequence rule, Metropolis acceptance and the
even/odd neighbour exchange, one ``random.Random(replica_index)`` stream per replica re-seeded at every
exchange step.

What is different by design: the R chains advance in LOCK-STEP -- one proposal per replica, one batched
``score`` call for all of them, R Metropolis decisions -- instead of R forked Python workers.  Trajectories
are statistically equivalent, not draw-for-draw identical: the reference itself is not reproducible across
processes (it iterates over ``set`` objects of strings, whose order depends on PYTHONHASHSEED).

Two drivers, ``run_design`` (per-replica Python objects, ``energy_scores.ReplicaScorer``) and ``run_design_fast`` (numpy state,
native proposals / Metropolis, or the whole inner loop in ``Engine.mc_run[_cofold]``), on one frame: ``_setup`` (problem, options,
shards, ladder, main stream, initial sequence), ``_start``, ``_exchange_step`` (the single all-gather, the swaps, records, stop
rule) and ``_finish`` exist once; candidates are scored by ``energy_scores.score_arrays`` in both.

Alternative structures: "snake" moves (connected components of the pair graph of target + alternative structures
switch between their Watson-Crick colourings) as in the reference (:143-388, :1081-1095).

``-nd on`` (negative design) runs through both drivers (``run_design_fast(negative_design="on")``: the second-best fold of the
solved candidates per iteration, or inside the native loop), and so does ``-oa on`` (``run_design_fast(oligo="on")``: every
candidate folded against a copy of itself, ``Engine.self_dimer`` per iteration or inside the native loop); ``-acgu on``
(weighted letter choices) is available in the Python driver (``run_design``) only.

Sequence motifs (``-motifs KEY,VALUE,...``, ``motifs=`` of every driver: ``energy_scores.parse_motifs``): a motif that occurs in
a candidate adds its value to the score, last of all additions.  ``run_design`` searches with the reference's regular
expressions (``energy_scores.score_motifs``); ``run_design_fast`` and ``run_puzzle_batch`` with the native matcher
(``HostKernels.motif_score`` per iteration, or the engine's motif set -- ``Engine.set_motifs`` -- inside every native loop).

Accessible regions (an input block ``>accessible``, one strand): ``accessible_weight`` x the opening energy of the region
(``Engine.unpaired_free_energy``) comes after the motif term, in ``run_design`` and in ``run_design_fast``'s per-iteration loop
(no native loop, no lock-step batch yet); ``--accessibility W`` profiles every window of the reported sequences.

Two strands (hetero-dimer, ``-d on`` homodimer) run through both drivers; together with alternative structures through
``run_design`` only.

A set of puzzles (``--set a.txt b.txt ...``, ``run_puzzle_set(batched=True)``): the one-strand puzzles with plain brackets and
no alternative structures advance in lock-step in ``run_puzzle_batch`` -- the per-puzzle state code of ``run_design_fast``
(``_array_state`` and what follows it), one ragged scoring call per iteration for all of them (``Engine.mc_run_ragged``) --,
the others one after the other.
"""
import argparse
import random
import time
from types import SimpleNamespace

import numpy as np

from . import energy_scores as es
from . import replica_exchange as rx
from .sim_score import pair_table

IUPAC = {
    'N': ['A', 'C', 'G', 'U'], 'W': ['A', 'U'], 'S': ['C', 'G'], 'M': ['A', 'C'], 'K': ['G', 'U'],
    'R': ['A', 'G'], 'Y': ['C', 'U'], 'B': ['C', 'G', 'U'], 'D': ['A', 'G', 'U'], 'H': ['A', 'C', 'U'],
    'V': ['A', 'C', 'G'], 'C': ['C'], 'A': ['A'], 'G': ['G'], 'U': ['U'], '&': ['&'],
}
CAN_PAIR = {'A': ['U'], 'U': ['G', 'A'], 'G': ['U', 'C'], 'C': ['G']}
WC = {'A': 'U', 'U': 'A', 'G': 'C', 'C': 'G'}


def parse_accessible(line, sec_struct):
    """the ``>accessible`` line of an input: as long as sec_struct, ``x`` = a position of the region that should be free (unpaired
    in the ensemble, not only in the MFE structure), ``.`` = the rest.  Returns the line; ValueError names what is wrong with it"""
    if "&" in sec_struct:
        raise ValueError("accessible: a two-strand input has no accessible region yet (one strand only)")
    bad = sorted(set(line) - set("x."))
    if bad:
        raise ValueError("accessible: character %r (the line holds 'x' for the region and '.' for the rest)" % bad[0])
    if len(line) != len(sec_struct):
        raise ValueError("accessible: %d characters for a structure of %d. Check input file." % (len(line), len(sec_struct)))
    if "x" not in line:
        raise ValueError("accessible: no 'x' in the line, the region is empty")
    return line


def read_input(path):
    """``>key`` block format of the reference (name, seq_restr, sec_struct, optional seed_seq / alt_sec_struct), and the optional
    block ``>accessible`` (:func:`parse_accessible`): inp.accessible is its line, or None"""
    with open(path, encoding='utf-8') as fh:
        text = fh.read()
    data = {}
    for block in text.lstrip(">").rstrip("\n").split("\n>"):
        lines = block.split("\n")
        data[lines[0]] = lines[1:]
    inp = SimpleNamespace(name=data['name'][0], sec_struct=data['sec_struct'][0].strip(),
                          seq_restr=data['seq_restr'][0].strip(), seed_seq=None, alt_sec_struct=None, alt_sec_structs=None,
                          accessible=None)
    if 'seed_seq' in data:
        inp.seed_seq = data['seed_seq'][0].strip()
    if 'alt_sec_struct' in data:
        inp.alt_sec_structs = [x.strip() for x in data['alt_sec_struct']]
        inp.alt_sec_struct = inp.alt_sec_structs[0]
    if 'accessible' in data:
        inp.accessible = parse_accessible(data['accessible'][0].strip() if data['accessible'] else "", inp.sec_struct)
    return inp


class DesignProblem:
    """Target structure + restraints -> per-position letter sets and pairing partners (reference get_nt_list)."""

    def __init__(self, sec_struct, seq_restr=None, alt_sec_structs=None, acgu=None):
        # acgu: None (= -acgu off) or the nucleotide percentages of -acgu on, e.g. {'A': 15, 'C': 30, 'G': 30, 'U': 15}:
        # weighted letter choices in the initial sequence and in pair moves (reference :725-741, :1052-1064)
        self.acgu = acgu
        # two strands: the '&' stays in every string as a fixed, unpaired "letter" exactly as in the reference (its positions
        # count; seq_restr carries it too), so indices, windows and draw counts are the reference's
        self.two_strands = "&" in sec_struct
        self.sec_struct = sec_struct
        n = len(sec_struct)
        self.seq_restr = seq_restr or "N" * n
        if len(self.seq_restr) != n:
            raise ValueError("Secondary structure and sequence restraints are of different length. Check input file.")
        self.partner = pair_table(sec_struct).copy()          # all bracket families count as design pairs
        self.target_pairs = {(i, int(p)) for i, p in enumerate(self.partner) if p > i}
        self.pairs = set(self.target_pairs)
        self.snakes = []                                      # [(positions, [state strings])]
        self.snake_of = [-1] * n
        if alt_sec_structs:
            self._build_snakes(alt_sec_structs)
        letters = []
        for ch in self.seq_restr:
            if ch not in IUPAC:
                raise ValueError("Not allowed characters in sequence restraints. Check input file.")
            letters.append(list(IUPAC[ch]))
        allowed = [list(l) for l in letters]
        for i, j in self.pairs:
            pi = sorted({b for a in letters[j] for b in CAN_PAIR[a]} & set(letters[i]))
            pj = sorted({b for a in letters[i] for b in CAN_PAIR[a]} & set(letters[j]))
            if not pi or not pj:
                raise ValueError("Wrong restraints in the input file. Nucleotide %d %s, cannot pair with nucleotide %d %s"
                                 % (i + 1, letters[i], j + 1, letters[j]))
            allowed[i], allowed[j] = pi, pj
        self.letters, self.allowed = letters, allowed
        self.mutable = [i for i in range(n) if len(allowed[i]) != 1]
        self.n = n
        for k, (nodes, states) in enumerate(self.snakes):
            ok = [st for st in states if all(st[x] in letters[v] for x, v in enumerate(nodes))]
            if not ok:
                raise ValueError("The structural restraints are contradictive to sequence restraints. Check your input.")
            self.snakes[k] = (nodes, ok)

    def _build_snakes(self, alt_sec_structs):
        """Alternative structures (reference get_pairs_for_graphs / generate_graphs / update_graphs,
        utils/sequence_utils.py:143-388): the pairs of all structures form a graph; a pair with an end that
        also sits in another pair belongs to a "snake" (a connected component that must be two-coloured with one
        Watson-Crick letter pair: A/U, U/A, C/G or G/C); the remaining alternative pairs become ordinary design
        pairs.  State order follows the reference: colour 0 goes to the component's first vertex in the
        reference's traversal; both colourings are in the list, so only the order depends on it."""
        n = len(self.sec_struct)
        alt = set()
        for a in alt_sec_structs:
            if len(a) != n:
                raise ValueError("alternative structure and target are of different length")
            pt = pair_table(a)
            alt |= {(i, int(p)) for i, p in enumerate(pt) if p > i}
        merged = self.target_pairs | alt
        count = [0] * n
        for a, b in merged:
            count[a] += 1
            count[b] += 1
        graph_pairs = sorted(p for p in merged if count[p[0]] > 1 or count[p[1]] > 1)
        excluded = sorted(p for p in merged if not (count[p[0]] > 1 or count[p[1]] > 1))
        for a, b in excluded:                                 # ordinary pairs (the target's own ones are already there)
            self.pairs.add((a, b))
            self.partner[a], self.partner[b] = b, a
        adj = {}
        for a, b in graph_pairs:
            adj.setdefault(a, []).append(b)
            adj.setdefault(b, []).append(a)
        seen = set()
        comps = []
        for v in sorted(adj):
            if v in seen:
                continue
            colour = {v: 0}
            queue = [v]
            while queue:
                x = queue.pop(0)
                for y in adj[x]:
                    if y not in colour:
                        colour[y] = 1 - colour[x]
                        queue.append(y)
                    elif colour[y] == colour[x]:
                        raise ValueError("The structural restraints in the alternative structures cannot be solved. "
                                         "Check your input.")
            seen |= set(colour)
            nodes = sorted(colour)
            cols = [colour[x] for x in nodes]
            states = ["".join(m[c] for c in cols) for m in ("AU", "UA", "CG", "GC")]
            comps.append((nodes, states))
        comps.sort(key=lambda c: c[0][0])
        self.snakes = comps
        for k, (nodes, _) in enumerate(comps):
            for v in nodes:
                self.snake_of[v] = k

    def initial_sequence(self, rng):
        """reference initial_sequence_generator with -acgu off: unpaired -> A, first base of an unpaired stretch (length
        >= 2) after a paired base -> G (else U), pairs -> random G/C (else A/U) Watson-Crick pair, rest random."""
        n, part = self.n, self.partner
        s = list(self.seq_restr)
        for i in range(n):
            if part[i] < 0 and "A" in self.letters[i]:
                s[i] = "A"
        for i in range(1, n - 1):
            if part[i] < 0 and part[i - 1] >= 0 and part[i + 1] < 0:
                if "G" in self.letters[i]:
                    s[i] = "G"
                elif "U" in self.letters[i]:
                    s[i] = "U"
        for i, j in sorted(self.pairs):
            a, b = self.allowed[i], self.allowed[j]
            if self.acgu is not None:
                opts_i = sorted(a)
                s[i] = rng.choices(opts_i, weights=[self.acgu[x] for x in opts_i])[0]
                s[j] = WC[s[i]]
                continue
            if "C" in a and "G" in a and "C" in b and "G" in b:
                s[i] = rng.choice(["C", "G"]); s[j] = WC[s[i]]
            elif "C" in a and "G" in b:
                s[i], s[j] = "C", "G"
            elif "G" in a and "C" in b:
                s[i], s[j] = "G", "C"
            elif "A" in a and "U" in a and "A" in b and "U" in b:
                s[i] = rng.choice(["A", "U"]); s[j] = WC[s[i]]
            elif "A" in a and "U" in b:
                s[i], s[j] = "A", "U"
            elif "U" in a and "A" in b:
                s[i], s[j] = "U", "A"
            else:
                # restraints that only leave G-U wobble pairs (the reference falls through to unconstrained
                # random letters here): take any compatible pair
                s[i] = rng.choice(a)
                s[j] = rng.choice(sorted(set(b) & set(CAN_PAIR[s[i]])) or b)
        for i in range(n):
            if s[i] not in "ACGU":
                s[i] = rng.choice(IUPAC[s[i]])
        for nodes, states in self.snakes:                     # reference :750-760: every snake starts in its first state
            for x, v in enumerate(nodes):
                s[v] = states[0][x]
        return "".join(s)

    # ---- move set
    def mutation_position(self, mfe_ss, shelf_index, n_shelves, tm_max, tm_min, point_mutations, rng):
        if not point_mutations:
            return rng.choice(self.mutable)
        q = pair_table(mfe_ss)
        query = {(i, int(p)) for i, p in enumerate(q) if p > i}
        mutable = set(self.mutable)
        false_cases = {x for pr in (self.target_pairs - query) | (query - self.target_pairs) for x in pr if x in mutable}
        if not false_cases:
            return rng.choice(self.mutable)
        prob = round(float(np.linspace(tm_max, tm_min, num=n_shelves)[shelf_index]), 2)
        expanded = sorted({c + k for c in false_cases for k in range(-3, 4) if 0 < c + k <= self.n - 1})
        pool = rng.choices([expanded, self.mutable], weights=[prob, 1 - prob])[0]
        return rng.choice(pool)

    def mutate(self, seq, pos, rng, oligo_state="none"):
        """One move at `pos`; for homodimers the reference's strand-copy rules are applied afterwards (:1104-1126)."""
        out = self._mutate(seq, pos, rng)
        if oligo_state == "homodimer":
            j = int(self.partner[pos])
            ss1, ss2 = self.sec_struct.split("&")
            s1o, s2o = seq.split("&")
            s1m, s2m = out.split("&")
            if j >= 0 and self.snake_of[pos] < 0 and ss1 != ss2:
                d = sorted([pos, j])
                a, b = d[0], d[1] - len(s1o) - 1
                s1c = s1m[:b] + s2m[b] + s1m[b + 1:]
                s2c = s2m[:a] + s1m[a] + s2m[a + 1:]
                out = s1c + "&" + s2c
                s1m, s2m = s1c, s2c
            if ss1 == ss2:
                if s1m != s1o:
                    out = s1m + "&" + s1m
                elif s2m != s2o:
                    out = s2m + "&" + s2m
        return out

    def _mutate(self, seq, pos, rng):
        s = list(seq)
        j = int(self.partner[pos])
        if self.snake_of[pos] >= 0:                           # reference :1081-1095: move the whole snake to another state
            nodes, states = self.snakes[self.snake_of[pos]]
            x = nodes.index(pos)
            cur = next((st for st in states if st[x] == s[pos]), None)
            new_states = [st for st in states if st != cur]
            if new_states:
                st = rng.choice(new_states)
                for y, v in enumerate(nodes):
                    s[v] = st[y]
        elif j < 0:
            opts = [x for x in self.allowed[pos] if x != s[pos]] if len(self.allowed[pos]) > 1 else []
            if opts:
                s[pos] = rng.choice(opts)
        else:
            opts1 = sorted(x for x in self.allowed[pos] if x != s[pos]) if len(self.allowed[pos]) != 1 else list(self.allowed[pos])
            if self.acgu is not None:
                n1 = rng.choices(opts1, weights=[self.acgu[x] for x in opts1])[0]
            else:
                n1 = rng.choice(opts1)
            opts2 = sorted(set(self.allowed[j]) & set(CAN_PAIR[n1]))
            if opts2:
                if self.acgu is not None:
                    s[pos], s[j] = n1, rng.choices(opts2, weights=[self.acgu[x] for x in opts2])[0]
                else:
                    s[pos], s[j] = n1, rng.choice(opts2)
        return "".join(s)


def _sws_reached(simulation_data, num_results, oligo_state):
    """The reference's -sws test (utils/stats_inputs_outputs.py:240-264, run every 10th exchange step): records
    de-duplicated by sequence, sorted like the result file, cut to num_results -- stop when all of them are solved."""
    from . import outputs
    top = outputs.sort_and_filter(simulation_data, num_results, oligo_state=oligo_state)
    return len(top) == num_results and all(r["mcc"] == 0.0 for r in top)


def oligo_state_and_pks(sec_struct, dimer="off", oligo="off"):
    """reference DesiRNA.py:474-485: (oligo_state, pks) of a target from the -d / -oa switches and its bracket families"""
    if "&" in sec_struct:
        oligo_state = "homodimer" if dimer == "on" else "heterodimer"
    else:
        oligo_state = "avoid" if oligo == "on" else "none"
    return oligo_state, "on" if set(sec_struct) - set(".()&") else "off"


# ---- what run_design and run_design_fast share: set-up, the exchange step after the inner iterations, the final gather.  The
# drivers differ in their inner iterations and in how they hold the replica state only.

def _setup(input_file, replicas, steps, timelimit, t_min, t_max, scoring_f, seed, stop_when_solved, num_results, shards,
           dimer="off", oligo="off", subopt="off", acgu=None, keep_records=True, motifs=None, accessible_weight=1.0):
    """The run: problem, options, shards, temperature ladder, main stream and initial sequence (the same on every rank).
    `motifs`: the ``-motifs`` text or what ``energy_scores.parse_motifs`` makes of it; opts.motifs holds the latter, or None.
    opts.accessible: the input's ``>accessible`` region as a uint8 mask (None without the block), opts.accessible_weight its weight"""
    if isinstance(motifs, str):
        motifs = es.parse_motifs(motifs)
    region = getattr(input_file, "accessible", None)
    if region is not None:
        region = _engine_mask(parse_accessible(region, input_file.sec_struct))
        if not accessible_weight > 0:
            raise ValueError("accessible_weight must be > 0")
    prob = DesignProblem(input_file.sec_struct, input_file.seq_restr, input_file.alt_sec_structs, acgu=acgu)
    oligo_state, pks = oligo_state_and_pks(input_file.sec_struct, dimer, oligo)
    opts = SimpleNamespace(oligo_state=oligo_state, pks=pks, subopt=subopt, motifs=motifs or None, param="1999",
                           scoring_f=es.parse_scoring_functions(scoring_f), accessible=region,
                           accessible_weight=float(accessible_weight))
    shards = shards or rx.ReplicaShards(replicas, 0, 1)
    run = SimpleNamespace(prob=prob, opts=opts, shards=shards, local=shards.local, steps=steps, timelimit=timelimit,
                          stop_when_solved=stop_when_solved, num_results=num_results, keep_records=keep_records, step=0)
    run.temps = rx.get_rep_temps(replicas, t_min, t_max)       # temperature shelf of EVERY replica, replayed on every rank
    run.shelves = list(run.temps)
    # main stream (initial sequence, swap acceptance; DesiRNA.py:659-664): the same on every rank
    run.main_rng = random.Random(shards.broadcast_seed(2137 + seed if seed else random.random()))
    # input_file.seed_seq is read but ignored, as in the reference
    run.init = prob.initial_sequence(run.main_rng)
    return run


def _engine_mask(line):
    """an ``x`` / ``.`` line -> (1, n) uint8 mask of ``Engine.unpaired_free_energy``"""
    return np.array([[c == "x" for c in line]], dtype=np.uint8)


def _start(run, scores, solved, records):
    """After the initial sequence is scored: first records, counters, clock; a solved start is made known to every rank"""
    run.simulation_data = records() if run.keep_records else []        # reference DesiRNA.py:353: one record per replica and step
    run.stats = dict(acc_mc=0, acc_mc_better=0, rej_mc=0, acc_re=0, rej_re=0, scored=len(run.local))
    run.t_start = time.time()
    if run.shards.world > 1:
        _, ex = run.shards.allgather_scores(scores, extras=[float(solved)])
        solved = bool(ex[:, 0].any())
    run.solved = solved
    run.stop = run.stop_when_solved and solved and run.num_results is None


def _next_step(run):
    if run.stop or (run.steps is not None and run.step >= run.steps):
        return False
    run.step += 1
    return True


def _exchange_step(run, scores, any_solved, records):
    """Replica exchange after the inner iterations: ONE all-gather (this rank's scores + its control flags: solved, time is up
    -- rank 0's clock decides --, -sws reached), then every rank replays the same swaps on the whole ladder.  `records()` returns
    this rank's records (sim_step = step * exchange, reference DesiRNA.py:371-375) with the temperatures of run.temps."""
    flags = [float(any_solved), float(time.time() - run.t_start >= run.timelimit), 0.0]
    sws = run.stop_when_solved and run.num_results is not None
    if sws and run.keep_records and run.step % 10 == 0:
        flags[2] = float(_sws_reached(run.simulation_data + records(), run.num_results, run.opts.oligo_state))
    all_scores, ex = run.shards.allgather_scores(scores, extras=flags)
    run.solved = run.solved or bool(ex[:, 0].any())
    run.temps, acc, _, rej = rx.replica_exchange(list(run.temps), list(all_scores), run.step, run.main_rng)
    run.stats["acc_re"] += acc
    run.stats["rej_re"] += rej
    if run.keep_records:
        run.simulation_data += records()
    run.stop = bool(ex[0, 1]) or (run.stop_when_solved and (bool(ex[:, 2].all()) if sws else run.solved))


def _finish(run, best):
    """the best replica of the whole job, on every rank"""
    if run.shards.world > 1:
        cands = rx.gather_results({run.shards.rank: best}, run.shards.world)
        best = min((b for b in cands.values() if b is not None), key=lambda s: (s.mcc, s.scoring_function))
    run.stats["elapsed_s"] = time.time() - run.t_start
    return best


def run_design(input_file, replicas=10, exchange=100, steps=None, timelimit=60, t_min=10.0, t_max=150.0,
               scoring_f="Ed-Epf:1.0", tm_max=0.7, tm_min=0.0, point_mutations="on", seed=0, stop_when_solved=False,
               device=0, shards=None, scorer=None, progress=None, dimer="off", oligo="off", acgu=None, subopt="off",
               num_results=None, motifs=None, accessible_weight=1.0):
    """Replica-exchange Monte-Carlo design of one target.  Returns dict(best=ScoreSeq, solved=bool, history=..., stats=...).

    ``shards`` (a ``replica_exchange.ReplicaShards``) splits the replicas over ranks; every rank proposes and scores its
    own replicas; ONE all-gather per exchange step carries the scores (and the ranks' solved / time-is-up flags), then every
    rank replays the same swaps on the whole temperature ladder, which it tracks itself.  Stop decisions are collective:
    they are taken from the gathered flags (rank 0's clock decides the time limit), so no rank leaves the loop alone.

    Loop semantics of the reference (``DesiRNA.py:361-383``): the time limit holds also when ``steps`` is given; records
    carry ``sim_step = global_step * exchange``; ``stop_when_solved`` with ``num_results`` is the reference's ``-sws on``
    (every 10th step: stop when the best ``num_results`` distinct sequences are all solved), without it the run stops at the
    first solved replica (an extension used by the tests and by the puzzle-set driver).

    ``motifs`` (``-motifs``: the text ``"KEY,VALUE,..."`` or ``energy_scores.parse_motifs`` of it): the scorer adds the motif
    term to every candidate (``ReplicaScorer.score``).  A ``scorer`` handed in scores with its own ``sim_options``.

    An input with an ``>accessible`` region (one strand): every candidate's opening energy of the region,
    ``Eopen = F[region unpaired] - Epf`` (``Engine.unpaired_free_energy``, one call per batch), times ``accessible_weight`` is the
    last addition to its score, after the motif term; records carry ``opening_energy`` and ``p_unpaired``."""
    run = _setup(input_file, replicas, steps, timelimit, t_min, t_max, scoring_f, seed, stop_when_solved, num_results,
                 shards, dimer, oligo, subopt, acgu, motifs=motifs, accessible_weight=accessible_weight)
    prob, local = run.prob, run.local
    scorer = scorer or es.ReplicaScorer(input_file, run.opts, max_replicas=max(1, len(local)), device=device)
    cur = scorer.score([run.init] * len(local)) if local else []
    for k, r in enumerate(local):
        cur[k].get_replica_num(r + 1)

    def records():                                            # (also moves the replicas onto their shelves of run.temps)
        for k, r in enumerate(local):
            cur[k].get_temp_shelf(run.temps[r])
            cur[k].get_sim_step(run.step * exchange)
        return [dict(vars(s)) for s in cur]

    best = min(cur, key=lambda s: (s.mcc, s.scoring_function)) if cur else None
    _start(run, [s.scoring_function for s in cur], best is not None and best.mcc == 0.0, records)
    stats = run.stats
    while _next_step(run):
        rngs = [random.Random(r) for r in local]              # re-seeded with the replica index every exchange step
        for _ in range(exchange):
            props = []
            for k, r in enumerate(local):
                shelf = run.shelves.index(cur[k].temp_shelf)
                pos = prob.mutation_position(cur[k].mfe_ss, shelf, replicas, tm_max, tm_min, point_mutations == "on", rngs[k])
                props.append(prob.mutate(cur[k].sequence, pos, rngs[k], run.opts.oligo_state))
            cand = scorer.score(props)
            stats["scored"] += len(props)
            for k in range(len(local)):
                acc, better = rx.mc_delta(cur[k].scoring_function, cand[k].scoring_function, cur[k].temp_shelf, rngs[k])
                if acc:
                    cand[k].get_replica_num(cur[k].replica_num)
                    cand[k].get_temp_shelf(cur[k].temp_shelf)
                    cand[k].get_sim_step(run.step * exchange)
                    cur[k] = cand[k]
                    stats["acc_mc"] += 1
                    stats["acc_mc_better"] += int(better)
                    if (cur[k].mcc, cur[k].scoring_function) < (best.mcc, best.scoring_function):
                        best = cur[k]
                else:
                    stats["rej_mc"] += 1
        _exchange_step(run, [s.scoring_function for s in cur], any(s.mcc == 0.0 for s in cur), records)
        if progress:
            progress(run.step, best, stats)
    best = _finish(run, best)
    return {"best": best, "solved": run.solved, "replicas": cur, "stats": stats, "steps": run.step, "temps": list(run.temps),
            "simulation_data": run.simulation_data, "engine": getattr(scorer, "engine", None)}


# ---- what run_design_fast and run_puzzle_batch share: one puzzle's replica state in arrays, and what an inner iteration or a
# native call does to it.

def _array_state(run, b, exchange, two=False, oa=False, nd=False, region=False):
    """The replica state of one run: the arrays of the scored batch `b` (``energy_scores.score_arrays`` of the initial
    sequence) that ``Engine.mc_run*`` holds, under its names; the best state; the records.  Calls ``_start``."""
    Rl, local = len(run.local), np.array(run.local, dtype=np.int64)
    keys = (["seqs", "mfe_ss", "score", "mcc1", "Epf", "Ed"] + ["oligo_fraction", "bonus"] * (two or oa) + ["subopt_e"] * nd
            + ["opening_energy", "p_unpaired"] * region)
    cur = SimpleNamespace(**{k: np.array(getattr(b, k), dtype=np.uint8 if k in keys[:2] else np.float64) for k in keys})
    bonus_name = "monomer_bonus" if oa else "oligomer_bonus"
    if oa:
        cur.bonus_field = bonus_name                      # (energy_scores.record names the bonus of its records by it)
    # fields of `best`; after the strings, in the order of mc_run's best["vals"] (esubopt_minus_Epf follows from them)
    fields = (["sequence", "mfe_ss", "mcc", "scoring_function", "Epf", "edesired"] + ["oligo_fraction", bonus_name] * (two or oa)
              + ["subopt_e", "esubopt_minus_Epf"] * nd + ["opening_energy", "p_unpaired"] * region)
    st = SimpleNamespace(keys=keys, cur=cur, nd=nd, Rl=Rl, local=local, vals=[f for f in fields[2:] if f != "esubopt_minus_Epf"])

    def best_of(k):
        sc = es.record(cur, k)
        return SimpleNamespace(**{f: getattr(sc, f) if f in fields[:2] else float(getattr(sc, f)) for f in fields})

    def records():
        out = []
        for k in range(Rl):
            sc = es.record(cur, k)
            sc.get_replica_num(int(local[k]) + 1)
            sc.get_temp_shelf(float(run.temps[local[k]]))
            sc.get_sim_step(run.step * exchange)          # reference: stats.step = global_step * RE_attempt
            out.append(dict(vars(sc)))
        return out

    st.best_of, st.records = best_of, records
    st.best = best_of(int(np.lexsort((cur.score, cur.mcc1))[0]))
    _start(run, cur.score[:Rl], st.best.mcc == 0.0, records)
    return st


def _step_ladder(run, st, hk, rng_state, shelves):
    """Start of an exchange step: random.seed(replica index) for every local replica (App. C2) into `rng_state`; returns the
    replicas' temperatures and shelf indices"""
    hk.rng_seed(st.local if st.Rl else [0], out=rng_state)
    tl = np.array(run.temps, dtype=np.float64)[st.local if st.Rl else [0]]
    return tl, np.searchsorted(shelves, tl).astype(np.int32)


def _native_best(st):
    """`best` of ``Engine.mc_run*``: the best state going into a native call"""
    return dict(seq=np.frombuffer(st.best.sequence.encode(), dtype=np.uint8).copy(),
                ss=np.frombuffer(st.best.mfe_ss.encode(), dtype=np.uint8).copy(),
                vals=np.array([getattr(st.best, f) for f in st.vals], dtype=np.float64))


def _native_done(run, st, seq, ss, vals, counters, n_iter):
    """... and what comes back from it: the best state, the three counters"""
    st.best = SimpleNamespace(sequence=seq.tobytes().decode(), mfe_ss=ss.tobytes().decode(),
                              **{f: float(v) for f, v in zip(st.vals, vals)})
    if st.nd:
        st.best.esubopt_minus_Epf = st.best.subopt_e - st.best.Epf if st.best.mcc == 0 else 0.0
    stats = run.stats
    stats["acc_mc"] += int(counters[0]); stats["acc_mc_better"] += int(counters[1]); stats["rej_mc"] += int(counters[2])
    stats["scored"] += st.Rl * n_iter


def _host_accept(run, st, p, acc, better):
    """One iteration's Metropolis outcome on the state: the accepted candidates of the scored batch `p` replace their replicas"""
    cur, stats = st.cur, run.stats
    for k in st.keys:
        getattr(cur, k)[acc] = getattr(p, k)[acc]
    na = int(acc.sum())
    stats["acc_mc"] += na
    stats["acc_mc_better"] += int((acc & better).sum())
    stats["rej_mc"] += st.Rl - na
    stats["scored"] += st.Rl
    # the best state is tracked replica by replica in replica order, like the native loop (first strictly better wins)
    for kb in np.nonzero(acc)[0]:
        if (cur.mcc1[kb], cur.score[kb]) < (st.best.mcc, st.best.scoring_function):
            st.best = st.best_of(kb)


def _array_exchange(run, st):
    _exchange_step(run, st.cur.score[:st.Rl], bool(st.Rl) and bool((st.cur.mcc1[:st.Rl] == 0.0).any()), st.records)


def _array_result(run, st, eng, native_loop):
    best = _finish(run, st.best if st.Rl else None)
    return {"best": best, "solved": run.solved, "stats": run.stats, "steps": run.step, "simulation_data": run.simulation_data,
            "engine": eng, "temps": [float(t) for t in run.temps], "local": [int(r) for r in st.local],
            "used_native_loop": bool(native_loop)}


def run_design_fast(input_file, replicas=10, exchange=100, steps=None, timelimit=60, t_min=10.0, t_max=150.0,
                    scoring_f="Ed-Epf:1.0", tm_max=0.7, tm_min=0.0, point_mutations="on", seed=0, stop_when_solved=False,
                    device=0, engine=None, keep_records=True, native_loop=None, shards=None, num_results=None, dimer="off",
                    negative_design="off", oligo="off", motifs=None, accessible_weight=1.0):
    """Same loop as :func:`run_design` with the per-replica host work in native code and no per-step Python objects:
    proposals, SimScore and Metropolis run batched in the C library, the replica state lives in numpy arrays (the batch of
    ``energy_scores.score_arrays``, of which it keeps what ``Engine.mc_run`` holds).  The
    per-replica random streams are the reference's (MT19937 seeded with the replica index at every exchange step, CPython's
    draw mapping: ``host_driver.hpp``), so for a fixed seed this driver and :func:`run_design` walk the same trajectory.

    ``shards`` (``replica_exchange.ReplicaShards``): this rank holds replicas ``shards.local`` only (its engine needs
    ``max_R >= len(shards.local)``); per exchange step ONE all-gather carries the scores and the stop flags, every rank
    replays the swaps on the whole ladder.  Results do not depend on the sharding (streams are seeded by the GLOBAL
    replica index and the kernels' results do not depend on the batch composition).

    Two-strand targets (one ``&``; ``dimer="on"`` = homodimer, else hetero-dimer) take ``HostKernels.propose_co`` and
    ``Engine.cofold_batch`` per iteration, or ``Engine.mc_run_cofold`` for the whole inner loop; their records carry the
    ``oligo_fraction`` and ``oligomer_bonus`` :func:`run_design` writes.  Alternative structures with two strands raise.

    ``negative_design="on"`` (``-nd on``, reference ``utils/energy_scores.py:104-108``): every solved candidate (1 - MCC == 0)
    loses ``subopt_e - Epf``, the second-best structure's energy from ``Engine.subopt_energy`` / ``Engine.cofold_subopt_energy``
    on the solved subset, or from the negative-design step of ``Engine.mc_run[_cofold]``; for two strands before the bonus.
    Records and ``best`` carry ``subopt_e`` and ``esubopt_minus_Epf`` as :func:`run_design`'s do.

    ``oligo="on"`` (``-oa on``, the reference's ``oligo_state == "avoid"``, ``utils/energy_scores.py:118-119``, ``:412-419``):
    every candidate is folded against a copy of itself (``Engine.self_dimer`` per iteration, or the self-dimer step of
    ``Engine.mc_run(self_dimer=True)``) and ``-kT ln(1 - oligo_fraction)`` is the last addition to its score, after the
    negative-design term.  Records and ``best`` carry ``oligo_fraction`` and ``monomer_bonus`` as :func:`run_design`'s do.  With a
    two-strand target the ``&`` decides, as in ``oligo_state_and_pks``: the switch is then without effect.

    ``motifs`` (``-motifs``: the text ``"KEY,VALUE,..."`` or ``energy_scores.parse_motifs`` of it; reference
    ``utils/energy_scores.py:121-123``): the motif term of every candidate's string (two strands: with its ``&``) is the last
    addition to its score, from ``HostKernels.motif_score`` per iteration or inside the native loop, which takes the set from
    the engine: the run sets it (``Engine.set_motifs``) before its first native call -- to the empty set when it has none, so
    that an engine handed in does not carry an earlier run's motifs into this one.  No column of its own in the records.

    An input with an ``>accessible`` region (one strand; :func:`run_design` has the rule): ``accessible_weight`` x the opening energy
    of the region is the last addition to every candidate's score, from one ``Engine.unpaired_free_energy`` call per iteration.
    The native loops do not know the term, so a region turns ``native_loop`` off; records and ``best`` carry ``opening_energy`` and
    ``p_unpaired``."""
    from . import engine as _engine
    if stop_when_solved and num_results is not None and not keep_records:
        raise ValueError("the -sws rule with num_results ranks the recorded sequences: it needs keep_records=True "
                         "(without records the stop test could never fire and the run would only end at its step / time limit)")
    two = "&" in input_file.sec_struct
    if two and input_file.alt_sec_structs:
        raise NotImplementedError("two strands with alternative structures run through run_design (the native two-strand "
                                  "proposer has no snake moves)")
    es.check_scoring_functions(es.parse_scoring_functions(scoring_f))
    run = _setup(input_file, replicas, steps, timelimit, t_min, t_max, scoring_f, seed, stop_when_solved, num_results,
                 shards, dimer, oligo, keep_records=keep_records, motifs=motifs, accessible_weight=accessible_weight)
    prob, sf, oligo_state, nd = run.prob, run.opts.scoring_f, run.opts.oligo_state, negative_design == "on"
    region = run.opts.accessible
    oa = oligo_state == "avoid"
    R, L, Rl = replicas, prob.n, len(run.local)
    eng = engine or _engine.Engine(max_R=max(1, Rl), max_L=L - 1 if two else L, device=device)      # L counts the '&'
    hk = _engine.HostKernels()
    eng.set_targets([input_file.sec_struct.replace("&", "")] + list(input_file.alt_sec_structs or []))
    score = lambda seqs_u8: es.score_arrays(eng, hk, input_file.sec_struct, sf, seqs_u8, oligo_state, run.opts.pks, nd, self_dimer=oa,
                                            motifs=run.opts.motifs,
                                            **(dict(accessible=region, accessible_weight=run.opts.accessible_weight)
                                               if region is not None else {}))
    st = _array_state(run, score(np.tile(np.frombuffer(run.init.encode(), dtype=np.uint8), (max(1, Rl), 1))), exchange, two, oa, nd,
                      region is not None)
    cur = st.cur
    if native_loop is None:
        native_loop = True
    if region is not None:
        native_loop = False                               # drna_mc_run* has no opening-energy step
    native_loop = native_loop and all(name in eng.TERM_IDS for name, _ in sf)   # (every -sf term, Edef included, has a native id)
    if native_loop and Rl:
        eng.set_motifs(run.opts.motifs)                   # this run's set or none: the engine may come from another run
    flags = _engine.NEED_PF | _engine.NEED_MFE | _engine.NEED_EVAL | (_engine.NEED_PK if run.opts.pks == "on" else 0)
    rng_state = np.empty((max(1, Rl), _engine.RNG_WORDS), dtype=np.uint32)
    shelves = np.array(run.shelves)
    targeted = point_mutations == "on"
    while _next_step(run):
        tl, shelf_idx = _step_ladder(run, st, hk, rng_state, shelves)
        if native_loop and Rl:
            # the whole inner loop of the exchange step in native code (drna_mc_run[_cofold]): one call, no per-iteration Python
            counters = np.zeros(3, dtype=np.int64)
            nd_kw = dict(subopt_e=cur.subopt_e) if nd else {}
            bst = _native_best(st)
            if two:
                eng.mc_run_cofold(prob, oligo_state, exchange, shelf_idx, R, tm_max, tm_min, targeted, tl, sf, rng_state, vars(cur),
                                  counters, bst, **nd_kw)
            else:
                eng.mc_run(prob, exchange, shelf_idx, R, tm_max, tm_min, targeted, tl, sf, flags, rng_state, vars(cur), counters, bst,
                           **nd_kw, **(dict(self_dimer=True) if oa else {}))
            _native_done(run, st, bst["seq"], bst["ss"], bst["vals"], counters, exchange)
        for _ in range(0 if (native_loop or not Rl) else exchange):
            if two:
                prop = hk.propose_co(prob, oligo_state, cur.seqs, cur.mfe_ss, shelf_idx, R, tm_max, tm_min, targeted, rng_state)
            else:
                prop = hk.propose_alt(prob, cur.seqs, cur.mfe_ss, shelf_idx, R, tm_max, tm_min, targeted, rng_state)
            p = score(prop)
            acc, better = hk.metropolis(cur.score, p.score, tl, rng_state)
            _host_accept(run, st, p, acc, better)
        _array_exchange(run, st)
    return _array_result(run, st, eng, native_loop)


class _RaggedSlice:
    """One puzzle's part of a ragged scoring call, as the engine ``energy_scores.score_arrays`` asks: the -sf sum stays there"""

    def __init__(self, Epf, Emfe, ss, Ed, edef=None, eng=None):
        self.out = (Epf, Emfe, ss, Ed.reshape(-1, 1))
        self.edef, self.eng = edef, eng

    def score_batch_arrays(self, seqs_u8, flags=0):
        return self.out

    def ensemble_defect_arrays(self, seqs_u8):
        return self.edef                                  # the puzzle's part of the set's one ragged ensemble-defect call

    def subopt_energy(self, seqs):
        return self.eng.subopt_energy(seqs)               # the solved candidates of ONE puzzle: equal lengths, the uniform call


def batch_eligible(input_file, scoring_f="Ed-Epf:1.0", negative_design="off", oligo="off", subopt="off", acgu=None, **_):
    """Can this input run in :func:`run_puzzle_batch` under these driver keywords?  One strand, the brackets ``( ) .`` only, no
    alternative structures, no ``>accessible`` region; -nd, -oa and -acgu off; no Edef term."""
    return (set(input_file.sec_struct) <= set("().") and not input_file.alt_sec_structs and negative_design == "off"
            and getattr(input_file, "accessible", None) is None
            and oligo == "off" and subopt == "off" and acgu is None
            and all(name != "Edef" for name, _ in es.parse_scoring_functions(scoring_f)))


def run_puzzle_batch(inputs, replicas=10, exchange=100, steps=None, timelimit=60, t_min=10.0, t_max=150.0,
                     scoring_f="Ed-Epf:1.0", tm_max=0.7, tm_min=0.0, point_mutations="on", seed=0, stop_when_solved=False,
                     device=0, engine=None, keep_records=True, native_loop=None, num_results=None, dimer="off",
                     negative_design="off", oligo="off", motifs=None):
    """:func:`run_design_fast` for a SET of puzzles of different lengths on one engine, all advancing in lock-step: per
    iteration the chains of every puzzle still running are scored by ONE ragged call (``Engine.mc_run_ragged`` runs the whole
    exchange step; with ``native_loop=False`` per iteration ``HostKernels.propose_alt`` per puzzle, one
    ``Engine.score_ragged_arrays`` call, ``HostKernels.metropolis`` per puzzle).  Returns one result dict per input, in input
    order, with :func:`run_design_fast`'s keys.

    ``negative_design="on"`` and an ``Edef`` term run in lock-step, too (``Engine.mc_run_ragged_nd``): per iteration one ragged
    ensemble-defect pass over all chains, and the solved proposals of all puzzles in one ragged second-best launch set.  With
    ``native_loop=False`` (a diagnostic path) the ensemble defect is one ``Engine.ensemble_defect_ragged_arrays`` call per
    iteration; the second-best energies are one ``Engine.subopt_energy`` call per puzzle with solved candidates.  Records and
    ``best`` carry ``subopt_e`` / ``esubopt_minus_Epf`` and ``Edef`` as :func:`run_design_fast`'s do.

    ``motifs`` as in :func:`run_design_fast`, the same set for every puzzle: per iteration ``HostKernels.motif_score`` per puzzle,
    or the engine's set (``Engine.set_motifs``, set or cleared before the first native call) inside the lock-step loops.

    Every puzzle is a run of its own -- main stream, temperature ladder, replica streams, records, exchange step and stop rule
    are those of :func:`run_design_fast` --, and the kernels' results do not depend on the batch composition: for the same
    keywords a puzzle's records, counters and best are those of its run alone.  A puzzle whose run stops (its step count,
    ``stop_when_solved``, the ``-sws`` rule) leaves the batch; the next call holds fewer chains.

    Lock-step ties every puzzle to the pace of the longest one still running.  ``timelimit``: every run's clock starts when the
    SET starts, so the limit bounds the whole set, not each puzzle in turn; ``steps`` is the deterministic mode.

    Inputs: one strand, the brackets ``( ) .`` only, no alternative structures, ``oligo="off"``: the ragged evaluation holds
    one structure per sequence and the loop has no self-dimer step.  (:func:`batch_eligible`, which routes ``--set``, is narrower:
    it still sends ``-nd on`` and ``Edef`` sets to the per-puzzle driver.)  The engine needs ``max_R`` = the sum of all replicas
    and ``max_L`` = the longest puzzle.  No replica sharding here."""
    from . import engine as _engine
    if stop_when_solved and num_results is not None and not keep_records:
        raise ValueError("the -sws rule with num_results ranks the recorded sequences: it needs keep_records=True")
    bad = [i.name for i in inputs if not (set(i.sec_struct) <= set("().") and not i.alt_sec_structs and oligo == "off"
                                          and getattr(i, "accessible", None) is None)]
    if bad:
        raise ValueError("not a puzzle for the lock-step batch (still refused: two strands, brackets other than ( ) ., "
                         "alternative structures, an >accessible region, -oa on): %s" % ", ".join(bad))
    if not inputs:
        return []
    es.check_scoring_functions(es.parse_scoring_functions(scoring_f))
    if isinstance(motifs, str):
        motifs = es.parse_motifs(motifs)
    runs = [_setup(i, replicas, steps, timelimit, t_min, t_max, scoring_f, seed, stop_when_solved, num_results, None, dimer,
                   oligo, keep_records=keep_records, motifs=motifs) for i in inputs]
    P, R, sf = len(inputs), replicas, runs[0].opts.scoring_f
    nd, want_edef = negative_design == "on", any(name == "Edef" for name, _ in sf)
    eng = engine or _engine.Engine(max_R=P * R, max_L=max(r.prob.n for r in runs), device=device)
    hk = _engine.HostKernels()
    flags = _engine.NEED_PF | _engine.NEED_MFE | _engine.NEED_EVAL

    def score_all(act, seqs):
        """one ragged call over the (R, L_i) candidates `seqs` of the puzzles `act` -> their score_arrays batches"""
        flat = np.concatenate([s.ravel() for s in seqs])
        lens, tof = np.repeat([runs[i].prob.n for i in act], R), np.repeat(np.array(act, dtype=np.int32), R)
        Epf, Emfe, ss, Ed = eng.score_ragged_arrays(flat, lens, tof, flags)
        edef = eng.ensemble_defect_ragged_arrays(flat, lens, tof) if want_edef else None      # ONE call for all active puzzles
        out, o = [], 0
        for k, (i, s) in enumerate(zip(act, seqs)):
            n, rows = R * runs[i].prob.n, slice(k * R, (k + 1) * R)
            part = _RaggedSlice(Epf[rows], Emfe[rows], ss[o:o + n].reshape(R, -1), Ed[rows], edef[rows] if want_edef else None, eng)
            out.append(es.score_arrays(part, hk, inputs[i].sec_struct, sf, s, "none", "off", nd, motifs=runs[i].opts.motifs))
            o += n
        return out

    eng.set_targets_ragged([i.sec_struct for i in inputs])      # target_of = the input's index, whatever the active set
    init = score_all(list(range(P)), [np.tile(np.frombuffer(r.init.encode(), dtype=np.uint8), (R, 1)) for r in runs])
    sts = [_array_state(run, b, exchange, False, False, nd) for run, b in zip(runs, init)]
    t0 = time.time()
    for run in runs:
        run.t_start = t0                                        # one clock for the set
    if native_loop is None:
        native_loop = True
    aux = nd or want_edef                                       # the loop with the auxiliary folds (drna_mc_run_ragged_nd)
    native_loop = bool(native_loop and hasattr(eng, "mc_run_ragged_nd" if aux else "mc_run_ragged")
                       and all(name in eng.TERM_IDS for name, _ in sf))
    if native_loop:
        eng.set_motifs(runs[0].opts.motifs)                     # the set's motifs or none: the engine may come from another run
    rng_state = np.empty((P * R, _engine.RNG_WORDS), dtype=np.uint32)
    targeted = point_mutations == "on"
    act = list(range(P))
    while True:
        act = [i for i in act if _next_step(runs[i])]           # who stopped has left the batch
        if not act:
            break
        A = len(act)
        lad = [_step_ladder(runs[i], sts[i], hk, rng_state[k * R:(k + 1) * R], np.array(runs[i].shelves)) for k, i in enumerate(act)]
        if native_loop:
            # the whole exchange step of every active puzzle in ONE native call (drna_mc_run_ragged[_nd])
            state = {k: np.concatenate([getattr(sts[i].cur, k).ravel() for i in act]) for k in sts[0].keys}
            bsts = [_native_best(sts[i]) for i in act]
            best = {k: np.concatenate([b[k] for b in bsts]) for k in ("seq", "ss")}
            best["vals"] = np.stack([b["vals"] for b in bsts])
            counters = np.zeros((A, 3), dtype=np.int64)
            args = ([runs[i].prob for i in act], exchange, np.concatenate([l[1] for l in lad]), [R] * A, tm_max, tm_min, targeted,
                    np.concatenate([l[0] for l in lad]), sf, flags, rng_state[:A * R], state, counters, best)
            if aux:
                eng.mc_run_ragged_nd(*args, subopt_e=state["subopt_e"] if nd else None)
            else:
                eng.mc_run_ragged(*args)
            o = ob = 0
            for k, i in enumerate(act):
                n, cur = runs[i].prob.n, sts[i].cur
                for key in sts[i].keys:
                    a = state[key]
                    getattr(cur, key)[...] = a[o:o + R * n].reshape(R, n) if key in ("seqs", "mfe_ss") else a[k * R:(k + 1) * R]
                _native_done(runs[i], sts[i], best["seq"][ob:ob + n], best["ss"][ob:ob + n], best["vals"][k], counters[k], exchange)
                o += R * n
                ob += n
        for _ in range(0 if native_loop else exchange):
            props = [hk.propose_alt(runs[i].prob, sts[i].cur.seqs, sts[i].cur.mfe_ss, lad[k][1], R, tm_max, tm_min, targeted,
                                    rng_state[k * R:(k + 1) * R]) for k, i in enumerate(act)]
            for k, (i, p) in enumerate(zip(act, score_all(act, props))):
                acc, better = hk.metropolis(sts[i].cur.score, p.score, lad[k][0], rng_state[k * R:(k + 1) * R])
                _host_accept(runs[i], sts[i], p, acc, better)
        for i in act:
            _array_exchange(runs[i], sts[i])
    return [_array_result(run, st, eng, native_loop) for run, st in zip(runs, sts)]


def run_puzzle_set(inputs, rank=0, world=1, driver=None, batched=False, on_result=None, **kw):
    """Design every problem of `inputs` (BASELINE config 4), the set sharded over `world` ranks by sum n^3
    (``replica_exchange.shard_puzzles``): each rank runs its own puzzles with all their replicas on its GPU and the
    results are gathered once at the end.  Returns {index: dict(name, solved, sequence, mfe_ss, score)} on every rank.

    ``batched=True``: the rank's puzzles that pass :func:`batch_eligible` under `kw` advance together in ONE
    :func:`run_puzzle_batch` (lock-step, one ragged scoring call per iteration); the others (two strands, alternative
    structures, pseudoknot brackets, -nd / -oa / -acgu on, an Edef term) go through `driver` one after the other as without it.
    ``on_result(index, input, result)`` is called with every full result of this rank (the CLI writes its files there)."""
    driver = driver or run_design_fast
    owner = rx.shard_puzzles([len(i.sec_struct) for i in inputs], world)
    own = [k for k in range(len(inputs)) if owner[k] == rank]
    together = [k for k in own if batched and batch_eligible(inputs[k], **kw)]
    results = dict(zip(together, run_puzzle_batch([inputs[k] for k in together], **kw))) if together else {}
    mine = {}
    for k in own:
        inp = inputs[k]
        res = results[k] if k in results else driver(inp, **kw)
        if on_result:
            on_result(k, inp, res)
        b = res["best"]
        mine[k] = dict(name=inp.name, solved=bool(res["solved"]), sequence=b.sequence, mfe_ss=b.mfe_ss,
                       score=float(b.scoring_function), rank=rank)
    return rx.gather_results(mine, world)


def _cli_driver(a, inp):
    """(driver, its keywords beyond the common ones) for one input under the command line `a`: the Python driver has -acgu and
    two strands together with alternative structures for itself"""
    strands2 = "&" in inp.sec_struct
    two = a.percs == "on" or (strands2 and bool(inp.alt_sec_structs))
    python_host = a.python_host or two
    if python_host:
        extra = dict(dimer=a.dimer, oligo=a.oligo, subopt=a.subopt) if (two or strands2 or a.subopt == "on" or a.oligo == "on") else {}
    else:
        extra = dict(dimer=a.dimer) if strands2 else {}
        if a.subopt == "on":
            extra["negative_design"] = "on"
        if a.oligo == "on":
            extra["oligo"] = "on"
    if a.percs == "on":
        vals = [int(x) for x in a.acgu_content.split(",")] if a.acgu_content else [15, 30, 30, 15]
        if sum(vals) != 100:
            raise SystemExit("The ACGU content should sum up to 100, check your command.")
        extra["acgu"] = dict(zip("ACGU", vals))
    if getattr(inp, "accessible", None) is not None:          # (only with the block: without it the drivers' keywords are as before)
        extra["accessible_weight"] = a.accessible_weight
    return (run_design if python_host else run_design_fast), extra


def ensemble_report(engine, result, input_file, S, top=5, seed=0):
    """Where the probability of each reported sequence goes: S structures per sequence drawn from its Boltzmann ensemble
    (``engine.sample_structures``, one call for the puzzle: the lengths are equal) and counted.  The reported sequences are
    ``result["reported"]`` (the ranked results the command line has just written) or, without it, the ranking of
    ``outputs.sort_and_filter`` over the run's records.  Returns the rows of ``<name>_ensemble.csv`` (``outputs.ENSEMBLE_COLUMNS``),
    per sequence: the ``top`` most frequent structures (kind ``top``, most frequent first, ties by string), a row for the target
    itself (kind ``target``, count 0 allowed; it repeats a ``top`` row when the target is one of them) and a row ``other`` with the
    samples that are neither among the top nor the target -- so top + other, plus target where it is not among the top, add up to S.
    Energies in kcal/mol (the target's, when it was not drawn, from the run's record of the sequence), 1 - MCC to the target by
    ``HostKernels.simscore``.  A two-strand design (an ``&`` in the target, the sequences ``'AAAA&BBBB'``) is sampled from the
    co-fold ensemble (``engine.cofold_sample_structures``): every structure compared and written keeps its ``&``, ``Epf`` is FAB,
    and 1 - MCC takes the ``&`` as ``Ee`` like every two-strand score."""
    from collections import Counter
    from . import engine as _engine
    from . import outputs
    target = input_file.sec_struct
    two = "&" in target
    seqs = list(result.get("reported") or [r["sequence"] for r in outputs.sort_and_filter(result["simulation_data"])])
    S, top = int(S), int(top)
    if two:
        ss, E, F4 = engine.cofold_sample_structures(seqs, S, seed)
        Epf = F4[:, 3]
    else:
        ss, E, Epf = engine.sample_structures(seqs, S, seed)
    hk = _engine.HostKernels()
    known = {r["sequence"]: r.get("edesired") for r in result.get("simulation_data") or []}
    rows = []
    for r, seq in enumerate(seqs):
        cnt = Counter(ss[r])
        energy = {s: int(E[r][k]) / 100.0 for k, s in enumerate(ss[r])}
        first = sorted(cnt, key=lambda s: (-cnt[s], s))[:top]
        listed = first + [target]
        sub = [s.replace("&", "Ee") for s in listed]         # the '&' -> 'Ee' substitution of every two-strand 1 - MCC
        mcc = 1.0 - hk.simscore(sub[-1], np.frombuffer("".join(sub).encode("ascii"), dtype=np.uint8).reshape(len(sub), -1))[0]
        row = lambda kind, rank, s, c, e, m: dict(sequence=seq, Epf=float(Epf[r]), kind=kind, rank=rank, structure=s, count=int(c),
                                                  frequency=c / S, energy=e, mcc=m)
        for k, s in enumerate(first):
            rows.append(row("top", k + 1, s, cnt[s], energy[s], float(mcc[k])))
        e_t = energy.get(target, known.get(seq))
        rows.append(row("target", "", target, cnt.get(target, 0), "" if e_t is None else float(e_t), float(mcc[-1])))
        rest = S - sum(cnt[s] for s in set(first) | {target})
        rows.append(row("other", "", "", rest, "", ""))
    return rows


def accessibility_report(engine, result, input_file, W):
    """How available every stretch of each reported sequence is: the opening energy ``Eopen = F[window unpaired] - Epf`` (kcal/mol)
    and ``p_unpaired = exp(-Eopen / kT)`` of every window of W nucleotides, start a = 1 .. n - W + 1 (1-based, ``end`` = a + W - 1
    inclusive), from ONE ``engine.unpaired_free_energy`` call per chunk of sequences with all n - W + 1 windows as its masks; Epf
    from the same chunk's score batch.  With an ``>accessible`` region in the input, its mask rides along as one more and gives the
    first row of each sequence (kind ``region``, start / end = its first / last ``x``).  The reported sequences are chosen as in
    :func:`ensemble_report`.  One strand.  Returns the rows of ``<name>_accessibility.csv`` (``outputs.ACCESSIBILITY_COLUMNS``)."""
    from . import engine as _engine
    from . import outputs
    if "&" in input_file.sec_struct:
        raise ValueError("the accessibility profile takes one strand")
    n, W = len(input_file.sec_struct), int(W)
    if not 1 <= W <= n:
        raise ValueError("window of %d nucleotides on a sequence of %d" % (W, n))
    seqs = list(result.get("reported") or [r["sequence"] for r in outputs.sort_and_filter(result["simulation_data"])])
    region = getattr(input_file, "accessible", None)
    masks = np.zeros((n - W + 1, n), dtype=np.uint8)
    for a in range(n - W + 1):
        masks[a, a:a + W] = 1
    spans = [("window", a + 1, a + W) for a in range(n - W + 1)]
    if region is not None:
        masks = np.concatenate([_engine_mask(region), masks])
        spans = [("region", region.index("x") + 1, region.rindex("x") + 1)] + spans
    step = max(1, int(getattr(engine, "max_R", len(seqs)) or len(seqs)))
    rows = []
    for r0 in range(0, len(seqs), step):           # (the scoring entry points take max_R sequences at a time)
        part = seqs[r0:r0 + step]
        Epf = engine.score_batch(part, _engine.NEED_PF)["Epf"]
        Eopen, p = engine.opening_energy(part, masks, Epf)
        for r, seq in enumerate(part):
            for m, (kind, start, end) in enumerate(spans):
                rows.append(dict(sequence=seq, kind=kind, start=start, end=end, opening_energy=float(Eopen[r, m]),
                                 p_unpaired=float(p[r, m])))
    return rows


KT_37 = 1.98717e-3 * 310.15          # kcal/mol at 37 C: the engine's partition functions are taken at this temperature


def structure_report(engine, result, input_file, gamma=1.0):
    """Which single structure stands for the ensemble of each reported sequence: beside the MFE structure the two predictors read
    from the pair probabilities, the centroid (the pairs with P > 1/2) and the maximum-expected-accuracy structure for the weight
    ``gamma`` (``engine.mea_structures``; two strands ``engine.cofold_mea_structures``; ViennaRNA's fc.centroid() and fc.MEA()).
    "MFE = target" with a centroid that is something else is the classic fragile design.  The reported sequences are chosen as in
    :func:`ensemble_report`.  Returns the rows of ``<name>_structures.csv`` (``outputs.STRUCTURE_COLUMNS``), three per sequence,
    ``kind`` = ``mfe``, ``centroid``, ``mea``: the structure, its energy in kcal/mol, ``Epf`` (two strands: FAB), its probability
    ``p_structure = exp(-(energy - Epf) / kT)``, ``value`` (blank / the centroid's expected base-pair distance to the ensemble /
    the MEA structure's expected accuracy) and ``mcc``, 1 - MCC to the target (``&`` -> ``Ee`` for two strands)."""
    import math
    from . import engine as _engine
    from . import outputs
    target = input_file.sec_struct
    two = "&" in target
    seqs = list(result.get("reported") or [r["sequence"] for r in outputs.sort_and_filter(result["simulation_data"])])
    step = max(1, int(getattr(engine, "max_R", len(seqs)) or len(seqs)))
    mfe_ss, Emfe, Epf = [], [], []
    for r0 in range(0, len(seqs), step):           # (the scoring entry points take max_R sequences at a time)
        part = seqs[r0:r0 + step]
        flags = _engine.NEED_PF | _engine.NEED_MFE
        out = engine.cofold_batch(part, flags) if two else engine.score_batch(part, flags)
        mfe_ss += list(out["mfe_ss"])
        Emfe += [int(x) for x in out["Emfe"]]
        Epf += [float(x) for x in (out["FAB"] if two else out["Epf"])]
    m = engine.cofold_mea_structures(seqs, gamma) if two else engine.mea_structures(seqs, gamma)
    hk = _engine.HostKernels()
    rows = []
    for r, seq in enumerate(seqs):
        listed = [mfe_ss[r], m["centroid"][r], m["mea"][r], target]
        sub = [s.replace("&", "Ee") for s in listed]         # the '&' -> 'Ee' substitution of every two-strand 1 - MCC
        mcc = 1.0 - hk.simscore(sub[-1], np.frombuffer("".join(sub).encode("ascii"), dtype=np.uint8).reshape(len(sub), -1))[0]
        energy = [Emfe[r] / 100.0, int(m["E"][r][1]) / 100.0, int(m["E"][r][0]) / 100.0]
        value = ["", float(m["centroid_distance"][r]), float(m["mea_value"][r])]
        for k, kind in enumerate(("mfe", "centroid", "mea")):
            rows.append(dict(sequence=seq, Epf=Epf[r], kind=kind, structure=listed[k], energy=energy[k],
                             p_structure=math.exp(-(energy[k] - Epf[r]) / KT_37), value=value[k], mcc=float(mcc[k])))
    return rows


def _cli_report(a, filename, inp, res):
    """What the command line leaves of one finished design: with -o the reference's result files (and, with --ensemble, the
    sampled ensemble of every reported sequence beside them; with --structures, their MFE, centroid and MEA structures), and the
    summary lines"""
    if a.outdir:
        import os
        from . import outputs
        os.makedirs(a.outdir, exist_ok=True)
        sf = es.parse_scoring_functions(a.scoring_f)
        oligo_state, pks = oligo_state_and_pks(inp.sec_struct, a.dimer, a.oligo)
        outname = outputs.get_outname(os.path.basename(filename), a.replicas, a.exchange, a.timlim, pks, "off", a.t_min, a.t_max,
                                      "1999", sf, "off", "off", a.pm)
        st = res["stats"]
        stats = SimpleNamespace(step=st["acc_mc"] + st["rej_mc"], global_step=res["steps"], acc_mc_step=st["acc_mc"],
                                acc_mc_better_e=st["acc_mc_better"], rej_mc_step=st["rej_mc"], acc_re_step=st["acc_re"],
                                rej_re_step=st["rej_re"])
        ranked, _ = outputs.write_all(res["simulation_data"], inp.name, os.path.basename(filename), outname, stats, st["elapsed_s"],
                                      a.timlim, time.strftime("%Y%m%d.%H%M%S"), num_results=a.num_results, directory=a.outdir,
                                      alt_sec_structs=list(inp.alt_sec_structs or []) or None, engine=res.get("engine"),
                                      oligo_state=oligo_state, subopt=a.subopt, sec_struct=inp.sec_struct)
        if a.ensemble:
            from . import engine as _engine
            eng = res.get("engine") or _engine.Engine(max_R=max(1, len(ranked)), max_L=len(inp.sec_struct))
            rows = ensemble_report(eng, dict(res, reported=[r["sequence"] for r in ranked]), inp, a.ensemble, a.ensemble_top,
                                   a.ensemble_seed)
            outputs.write_ensemble(rows, outname, a.outdir)
        if a.structures:
            from . import engine as _engine
            eng = res.get("engine") or _engine.Engine(max_R=max(1, len(ranked)), max_L=len(inp.sec_struct))
            rows = structure_report(eng, dict(res, reported=[r["sequence"] for r in ranked]), inp, a.structures)
            outputs.write_structures(rows, outname, a.outdir)
        if a.accessibility:
            from . import engine as _engine
            eng = res.get("engine") or _engine.Engine(max_R=max(1, len(ranked)), max_L=len(inp.sec_struct))
            rows = accessibility_report(eng, dict(res, reported=[r["sequence"] for r in ranked]), inp, a.accessibility)
            outputs.write_accessibility(rows, outname, a.outdir)
    b = res["best"]
    print("Design solved succesfully!" if res["solved"] else "Design not solved.")
    print(b.sequence)
    print(b.mfe_ss)
    print("Epf=%.3f Ed=%.3f 1-MCC=%.3f score=%.3f  steps=%d scored=%d in %.1fs" %
          (b.Epf, b.edesired, b.mcc, b.scoring_function, res["steps"], res["stats"]["scored"], res["stats"]["elapsed_s"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description="GPU replica-exchange RNA design (flag names follow DesiRNA.py)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("-f", "--filename", dest="name")
    src.add_argument("--set", nargs="+", dest="set_files", metavar="FILE", help="design all these inputs as one set: the puzzles "
                     "that allow it (one strand, ( ) . only, no alternative structures, -nd / -oa / -acgu off) advance in lock-step on "
                     "one engine, the others one after the other")
    ap.add_argument("-R", "--replicas", type=int, default=10)
    ap.add_argument("-e", "--exchange", type=int, default=100)
    ap.add_argument("-t", "--timelimit", type=int, default=60, dest="timlim")
    ap.add_argument("-s", "--steps", type=int, default=None)
    ap.add_argument("-tmin", "--tmin", type=float, default=10, dest="t_min")
    ap.add_argument("-tmax", "--tmax", type=float, default=150, dest="t_max")
    ap.add_argument("-sf", "--scoring_function", default="Ed-Epf:1.0", dest="scoring_f")
    ap.add_argument("-tm", "--target_mutations", default="on", choices=["off", "on"], dest="pm")
    ap.add_argument("-tm_perc_max", type=float, default=0.7, dest="tm_max")
    ap.add_argument("-tm_perc_min", type=float, default=0.0, dest="tm_min")
    ap.add_argument("-seed", "--seed_number", type=int, default=0, dest="in_seed")
    ap.add_argument("-sws", "--stop_when_solved", default="off", choices=["off", "on"], dest="sws")
    ap.add_argument("-r", "--results_number", type=int, default=10, dest="num_results")
    ap.add_argument("-d", "--dimer", default="off", choices=["off", "on"], dest="dimer", help="homodimer design (two-strand input)")
    ap.add_argument("-oa", "--avoid_oligomerization", default="off", choices=["off", "on"], dest="oligo")
    ap.add_argument("-nd", "--negative_design", default="off", choices=["off", "on"], dest="subopt")
    ap.add_argument("-acgu", "--ACGU", default="off", choices=["off", "on"], dest="percs", help="weighted nucleotide choices")
    ap.add_argument("-acgu_content", "--ACGU_content", default="", dest="acgu_content", help="A,C,G,U percentages (sum 100)")
    ap.add_argument("-motifs", "--motif_sequences", default=None, dest="motifs", help="Sequence motifs along with their "
                    "bonuses(-)/penalties(+). Provide comma-separated key,value,key,value sequence.")
    ap.add_argument("--python-host", action="store_true", help="per-replica Python host loop instead of the native batched one")
    ap.add_argument("-o", "--outdir", default=None, help="write the reference's result files (_results.csv, _traj.csv, "
                    "_stats, _best_str, fasta files) into this directory")
    ap.add_argument("--ensemble", type=int, default=0, metavar="S", help="after the run, draw S structures from the Boltzmann "
                    "ensemble of every reported sequence and write <name>_ensemble.csv beside _results.csv (needs -o; one strand)")
    ap.add_argument("--ensemble-top", type=int, default=5, metavar="T", help="structures listed per sequence, most frequent first")
    ap.add_argument("--ensemble-seed", type=int, default=0, help="seed of the samples (sequence r of the report: seed + r)")
    ap.add_argument("--structures", type=float, default=None, metavar="GAMMA", help="after the run, write the MFE, centroid and "
                    "maximum-expected-accuracy structure (weight GAMMA > 0) of every reported sequence into <name>_structures.csv "
                    "beside _results.csv (needs -o; one or two strands)")
    ap.add_argument("--accessible-weight", type=float, default=1.0, metavar="W", dest="accessible_weight", help="weight (> 0) of the "
                    "opening energy of an input's >accessible region in its scoring function")
    ap.add_argument("--accessibility", type=int, default=None, metavar="W", help="after the run, write the opening energy and the "
                    "probability of being unpaired of every window of W nucleotides (W >= 1) of every reported sequence into "
                    "<name>_accessibility.csv beside _results.csv (needs -o; one strand)")
    a = ap.parse_args(argv)
    if not a.accessible_weight > 0:
        ap.error("--accessible-weight takes a weight W > 0")
    if a.accessibility is not None and a.accessibility < 1:
        ap.error("--accessibility takes a window of W >= 1 nucleotides")
    if a.accessibility and not a.outdir:
        ap.error("--accessibility writes its file beside _results.csv: give -o")
    if a.structures is not None and not (a.structures > 0 and a.structures < float("inf")):
        ap.error("--structures takes a weight GAMMA > 0")
    if a.structures and not a.outdir:
        ap.error("--structures writes its file beside _results.csv: give -o")
    if a.ensemble < 0 or a.ensemble_top < 1:
        ap.error("--ensemble takes S >= 1 and --ensemble-top T >= 1")
    if a.ensemble and not a.outdir:
        ap.error("--ensemble writes its file beside _results.csv: give -o")
    common = dict(replicas=a.replicas, exchange=a.exchange, steps=a.steps, timelimit=a.timlim, t_min=a.t_min, t_max=a.t_max,
                  scoring_f=a.scoring_f, tm_max=a.tm_max, tm_min=a.tm_min, point_mutations=a.pm, seed=a.in_seed,
                  stop_when_solved=a.sws == "on", num_results=a.num_results if a.sws == "on" else None)
    if a.motifs is not None:                                      # (only with the flag: without it the drivers' keywords are as before)
        try:
            common["motifs"] = es.parse_motifs(a.motifs)
        except ValueError as err:
            ap.error(str(err))
    if a.set_files:
        inputs = [read_input(f) for f in a.set_files]
        if a.ensemble and any("&" in i.sec_struct for i in inputs):
            ap.error("--ensemble samples one strand: a two-strand input is refused")
        if a.accessibility and any("&" in i.sec_struct for i in inputs):
            ap.error("--accessibility profiles one strand: a two-strand input is refused")
        # the switches under run_design_fast's names, so that run_puzzle_set can tell which inputs may share the batch; the
        # per-puzzle driver gets each input's own keywords (_cli_driver)
        switches = dict(negative_design=a.subopt, oligo=a.oligo, **(dict(acgu=True) if a.percs == "on" or a.python_host else {}))

        def driver(inp, negative_design="off", oligo="off", acgu=None, **kw):
            drv, extra = _cli_driver(a, inp)
            return drv(inp, **extra, **kw)

        run_puzzle_set(inputs, driver=driver, batched=True, **common, **switches,
                       on_result=lambda k, inp, res: _cli_report(a, a.set_files[k], inp, res))
        return
    inp = read_input(a.name)
    if a.ensemble and "&" in inp.sec_struct:
        ap.error("--ensemble samples one strand: a two-strand input is refused")
    if a.accessibility and "&" in inp.sec_struct:
        ap.error("--accessibility profiles one strand: a two-strand input is refused")
    drv, extra = _cli_driver(a, inp)
    _cli_report(a, a.name, inp, drv(inp, **extra, **common))


if __name__ == "__main__":
    main()
