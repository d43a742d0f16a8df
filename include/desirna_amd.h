/*
 * desirna_amd.h -- C ABI of the MI355X (gfx950) replica-scoring engine.
 *
 * This is the drop-in boundary for the one hot path of fryzjergda/DesiRNA: scoring every mutated
 * sequence of every replica.  The reference has no FFI of its own; its de-facto operator boundary
 * is the set of ViennaRNA SWIG calls made per sequence by utils/energy_scores.py.
 * Each entry point below names the reference call sites it replaces (paths relative to the
 * reference tree).  Plain C types only; every buffer is owned by the caller; a handle is bound to
 * one GPU and must be used from one host thread at a time.
 *
 * Units: integer energies are dcal/mol (0.01 kcal/mol) exactly as ViennaRNA keeps them internally
 * (the Python shim divides by 100 to reproduce ViennaRNA's float returns); Epf is kcal/mol.
 * Sequences are upper- or lower-case A C G U (T is read as U); structures are dot-bracket strings
 * in which only '(' and ')' denote pairs for energy evaluation.
 */
#ifndef DESIRNA_AMD_H
#define DESIRNA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct drna_engine drna_engine;

/* Layout version of this interface.  Bumped whenever the meaning or size of a caller-owned buffer changes under an unchanged
 * symbol name (2 -> 3: rng_state of drna_propose_batch[_alt] / drna_metropolis_batch / drna_mc_run became R x DRNA_RNG_WORDS
 * uint32 MT19937 streams instead of R uint64).  A binding compares drna_abi_version() with the DRNA_ABI_VERSION it was written
 * against at load time, so a stale caller fails there instead of overrunning a buffer. */
#define DRNA_ABI_VERSION 3
int drna_abi_version(void);

/* return codes */
enum {
  DRNA_OK = 0,
  DRNA_ERR_ARG = -1,        /* null pointer, R/L out of range, bad flags                    */
  DRNA_ERR_PARAMS = -2,     /* malformed parameter blob                                     */
  DRNA_ERR_DEVICE = -3,     /* HIP error (no device, out of memory, launch failure)         */
  DRNA_ERR_SEQUENCE = -4,   /* a sequence holds a character other than A C G U T            */
  DRNA_ERR_STRUCTURE = -5,  /* unbalanced '(' ')' in a target structure                     */
  DRNA_ERR_PF_RANGE = -6,   /* partition function left the fp64 range despite scaling       */
  DRNA_ERR_INTERNAL = -7    /* traceback could not reproduce a table value (engine bug)     */
};

/* what drna_score_batch computes */
enum {
  DRNA_NEED_PF = 1u,          /* Epf            : fc.pf()            energy_scores.py:150           */
  DRNA_NEED_MFE = 2u,         /* mfe_ss + Emfe  : fc.mfe()           energy_scores.py:151, :354     */
  DRNA_NEED_PK = 4u,          /* pk annotation  : get_pk_struct()    sequence_utils.py:1166-1228    */
  DRNA_NEED_EVAL = 8u         /* Ed             : fc.eval_structure  energy_scores.py:75, :99       */
};

/*
 * Create an engine on HIP device `device`.
 * Replaces RNA.params_load(path) (DesiRNA.py:455-456) and the per-call table allocation of
 * RNA.fold_compound(seq, md) (energy_scores.py:147): parameters are expanded once into device
 * tables, workspaces are sized once for max_R sequences of at most max_L nucleotides.
 * `params` is the int32 blob produced by desirna_amd/params.py (layout documented there).
 */
int drna_create(const int32_t *params, int n_int32, int device, int max_R, int max_L, drna_engine **out);

void drna_destroy(drna_engine *e);

/* message for the last non-OK return on this engine (or for a failed drna_create when e == NULL) */
const char *drna_last_error(const drna_engine *e);

/*
 * Install the target structure(s) every sequence is evaluated against: targets[0] is the design
 * target (input file >sec_struct, '&' removed), targets[1..] the >alt_sec_struct lines.
 * Replaces the argument of fc.eval_structure(...) at energy_scores.py:75 and :99.
 * `targets` holds n_targets strings of exactly L characters, back to back (no terminators).
 */
int drna_set_targets(drna_engine *e, int n_targets, int L, const char *targets);

/*
 * Score R sequences of length L (host buffers).  Replaces, for all R replicas at once, the
 * ViennaRNA calls of score_sequence(): get_mfe_e_ss (energy_scores.py:128-159), eval_structure
 * (:75,:99), RNA.fold(seq)[1] (:354) and get_pk_struct (sequence_utils.py:1166-1228).
 *   seqs    R*L chars                                   in
 *   flags   OR of DRNA_NEED_*                           in
 *   Epf     R doubles, kcal/mol                         out (NEED_PF)      may be NULL otherwise
 *   Emfe    R int32, dcal/mol                           out (NEED_MFE)
 *   mfe_ss  R*L chars, no terminators                   out (NEED_MFE; pk-annotated with NEED_PK)
 *   Ed      R*n_targets int32, dcal/mol                 out (NEED_EVAL; needs drna_set_targets)
 */
int drna_score_batch(drna_engine *e, int R, int L, const char *seqs, uint32_t flags,
                     double *Epf, int32_t *Emfe, char *mfe_ss, int32_t *Ed);

/*
 * Same with every buffer already resident in device memory (e.g. torch tensors on the engine's
 * device).  Work is enqueued on the engine's streams and the call returns after they have drained.
 * status (device, R int32, may be NULL) receives per-sequence status words.
 */
int drna_score_batch_device(drna_engine *e, int R, int L, const char *d_seqs, uint32_t flags,
                            double *d_Epf, int32_t *d_Emfe, char *d_mfe_ss, int32_t *d_Ed);

/*
 * Timing hook for bench.py: average device time in milliseconds of the most recent
 * drna_score_batch*_ call, per kernel family, measured with HIP events on the engine's own
 * streams.  out[0] = MFE fill+traceback kernel, out[1] = PF kernel, out[2] = eval kernel,
 * out[3] = whole call (first launch to last completion).
 */
int drna_last_timing(const drna_engine *e, float out[4]);

/*
 * Ragged batches: sequences of DIFFERENT lengths scored in one call -- BASELINE config 4 (the 100 Eterna100-V1 puzzles,
 * 12 ... 400 nt, R replicas each) is one such batch instead of 100 calls.  The reference has no counterpart (it scores one
 * sequence per call); per sequence the results are those of drna_score_batch.
 *
 * drna_set_targets_ragged: n_targets structures of lengths lens[t], concatenated without terminators.
 * drna_score_ragged: R sequences of lengths lens[r], concatenated; target_of[r] names the structure E(target) is evaluated
 * on (same length; needed with DRNA_NEED_EVAL only).  Outputs: Epf R doubles, Emfe R int32, mfe_ss concatenated like the
 * sequences, Ed R int32 (ONE structure per sequence).  Sum of lengths <= max_R * max_L.
 */
int drna_set_targets_ragged(drna_engine *e, int n_targets, const int32_t *lens, const char *targets);
int drna_score_ragged(drna_engine *e, int R, const int32_t *lens, const char *seqs, const int32_t *target_of,
                      uint32_t flags, double *Epf, int32_t *Emfe, char *mfe_ss, int32_t *Ed);

/*
 * Two interacting strands (reference oligo_state homodimer / heterodimer, utils/energy_scores.py:154-158): R sequence
 * pairs of total length L, both strands concatenated WITHOUT the '&', the first strand `cut` nucleotides long.
 * Replaces fc.mfe_dimer() (structure + energy; the caller re-inserts the '&' at `cut`), fc.pf_dimer() (F4 = FA, FB, FcAB,
 * FAB in kcal/mol per pair; the reference's Epf is FAB = pf_dimer()[-1]; homodimer symmetry correction included) and the
 * two-strand fc.eval_structure (Ed against the structures of drna_set_targets, '&' removed, same cut).
 *   F4 R*4 doubles (NEED_PF), Emfe R int32 + mfe_ss R*L chars (NEED_MFE), Ed R*n_targets int32 (NEED_EVAL)
 */
int drna_cofold_batch(drna_engine *e, int R, int L, int cut, const char *seqs, uint32_t flags, double *F4,
                      int32_t *Emfe, char *mfe_ss, int32_t *Ed);

/*
 * Energy of the second-best structure of R sequences (negative design, -nd on).  Replaces
 * get_first_suboptimal_structure_and_energy(seq, fc, 1)[1] (utils/energy_scores.py:105-107, :453-488): ViennaRNA's subopt
 * enumeration with a growing energy band until it holds two structures, sorted by energy, second entry.
 *   E2   R int32, dcal/mol; 0 when no second structure lies within 4900 dcal/mol of the MFE (the reference's fallback)
 *   E12  R*2 int32, may be NULL: the two lowest structure energies (second = 10000000 if there is one structure only)
 */
int drna_subopt_energy_batch(drna_engine *e, int R, int L, const char *seqs, int32_t *E2, int32_t *E12);

/*
 * Energy of the second-best CO-FOLD structure of R sequence pairs (negative design with two strands, -nd on with an '&'
 * target).  Replaces get_first_suboptimal_structure_and_energy(seq, fc, 1)[1] on the dimer fold compound of the reference's
 * two-strand branch (utils/energy_scores.py:105-108, :453-488).  Pairs as for drna_cofold_batch: total length L, both
 * strands concatenated WITHOUT the '&', the first strand `cut` nucleotides long (1 <= cut < L).  The structures are those
 * of drna_cofold_batch's MFE (DuplexInit iff a pair joins the strands); two equal strands are not reduced by symmetry (a
 * structure and its rotation are two structures).
 *   E2   R int32, dcal/mol; 0 when no second structure lies within 4900 dcal/mol of the co-fold MFE (the reference's fallback)
 *   E12  R*2 int32, may be NULL: the two lowest structure energies (second = 10000000 if there is one structure only)
 */
int drna_cofold_subopt_energy_batch(drna_engine *e, int R, int L, int cut, const char *seqs, int32_t *E2, int32_t *E12);

/*
 * Base-pair probabilities and ensemble defect of R sequence pairs (two-strand -sf Edef): the reference's
 * ScoreSeq.get_ensemble_defect on a heterodimer / homodimer input (utils/energy_scores.py:93-94, :362-374; it pins no value
 * there).  Pairs as for drna_cofold_batch: total length L, both strands concatenated WITHOUT the '&', the first strand `cut`
 * nucleotides long (1 <= cut < L).  The ensemble is that of drna_cofold_batch's partition function: a structure weighs its
 * Boltzmann factor, times expDuplexInit if a pair joins the strands (halved when the two strands are the same sequence), so
 * the weights sum to exp(-FAB / kT).  P(i,j) = weight of the structures that hold the pair (i,j) / weight of all;
 * edef = (1/L) [ sum_{i unpaired in target} sum_j P(i,j) + sum_{i paired with m} (1 - P(i,m)) ] against targets[0] of
 * drna_set_targets (same L, '&' removed, '(' ')' pairs only).
 *   edef  R doubles
 *   bpp   R*(L+1)*(L+1) doubles, may be NULL: P(i,j) at [i*(L+1)+j], 1 <= i < j <= L, every other entry 0
 * R is not limited by max_R (chunks of max_R).  Pairs of at most "cofold_edef_lds_max" nucleotides take one fused launch with
 * every table in LDS (option "edef_lds", see drna_set_option); the values do not depend on it.
 * A new symbol: no existing buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_cofold_ensemble_defect_batch(drna_engine *e, int R, int L, int cut, const char *seqs, double *edef, double *bpp);

/*
 * The K lowest-energy structures of R sequences, energies and dot-bracket strings.  Replaces
 * get_first_suboptimal_structure_and_energy(seq, fc, k)[0] for k = 1 .. #alternative structures, the call behind
 * get_alt_mcc() (utils/sequence_utils.py:766-793, utils/energy_scores.py:453-488): entry k of ViennaRNA's energy-sorted
 * subopt list (uniq_ML = 1) is rank k here (rank 0 = a ground state).  Structures of equal energy come in this engine's
 * own fixed order (ViennaRNA's order among ties is pinned nowhere in the reference).  R is not limited by max_R (the
 * batch is worked off in chunks).
 *   K    1 .. 8
 *   E    R*K int32, dcal/mol, ascending per sequence; 10000000 where the sequence has fewer than rank+1 structures
 *   ss   R*K*L chars (no terminator); all dots where E = 10000000
 */
int drna_subopt_structs_batch(drna_engine *e, int R, int L, const char *seqs, int K, int32_t *E, char *ss);

/*
 * The K lowest-energy CO-FOLD structures of R sequence pairs, energies and dot-bracket strings: the final ranking of a
 * two-strand design with alternative structures.  Replaces get_first_suboptimal_structure_and_energy(seq, fc, k)[0] on the
 * dimer fold compound, the call behind get_alt_mcc() (utils/sequence_utils.py:766-793, utils/energy_scores.py:453-488) when
 * the sequence holds an '&'.  Pairs as for drna_cofold_batch: total length L, both strands concatenated WITHOUT the '&', the
 * first strand `cut` nucleotides long (1 <= cut < L).  The structures and energies are those of drna_cofold_batch's MFE and
 * of drna_cofold_subopt_energy_batch (DuplexInit iff a pair joins the strands; two equal strands are not reduced by symmetry:
 * a structure and its rotation are two structures), so E[0] is the co-fold MFE and E[0 .. 1] the E12 of that call.  The
 * reference pins no two-strand subopt output; structures of equal energy come in this engine's own fixed order.  R is not
 * limited by max_R (the batch is worked off in chunks).
 *   K    1 .. 8
 *   E    R*K int32, dcal/mol, ascending per pair; 10000000 where the pair has fewer than rank+1 structures
 *   ss   R*K*L chars (no terminator, no '&'); all dots where E = 10000000
 * A new symbol: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_cofold_subopt_structs_batch(drna_engine *e, int R, int L, int cut, const char *seqs, int K, int32_t *E, char *ss);

/*
 * Ensemble defect of R sequences against targets[0] (needs drna_set_targets with the same L): inside fill,
 * outside recursion, base-pair probabilities, then (1/L) * [ sum_{i unpaired in target} sum_j P(i,j)
 * + sum_{i paired with m in target} (1 - P(i,m)) ], '(' ')' pairs only.
 * Replaces ScoreSeq.get_ensemble_defect (energy_scores.py:362-374: new fold compound with bpp on, fc.mfe(),
 * fc.exp_params_rescale(mfe), fc.pf(), fc.ensemble_defect(target)); the rescale only moves pf_scale, which
 * cancels in every probability.
 *   edef  R doubles in [0,1]                                     out
 *   bpp   R*(L+1)*(L+1) doubles, P(i,j) at [r][i][j], 1 <= i < j <= L  out, may be NULL
 * R is not limited by max_R (chunks of max_R).  Sequences of at most "edef_lds_max" nucleotides take one fused launch with
 * every table in LDS (option "edef_lds", see drna_set_option).
 */
int drna_ensemble_defect_batch(drna_engine *e, int R, int L, const char *seqs, double *edef, double *bpp);

/* Same with device-resident buffers; d_bpp (may be NULL) must be zero-filled by the caller. */
int drna_ensemble_defect_batch_device(drna_engine *e, int R, int L, const char *d_seqs, double *d_edef,
                                      double *d_bpp);

/*
 * Stochastic traceback: S structures per sequence drawn from its Boltzmann ensemble (ViennaRNA's pbacktrack, RNAsubopt -p),
 * p(structure) = exp(-E / kT) / Z under the partition function's loop model.  One inside fill (pf_kernel) and one sample launch
 * per chunk of workspace slots: R is not limited by max_R.  One strand, equal lengths.
 *   S      >= 1 samples per sequence; R x S x L <= DRNA_SAMPLE_MAX_CHARS, beyond it DRNA_ERR_ARG
 *   seeds  R uint64.  Sample s of sequence r depends on the sequence, seeds[r] and s ALONE -- not on S, on R, on the neighbours in
 *          the batch or on the launch: the walk's draw k of sample s is u(seeds[r], s, k) of csrc/sample_rng.hpp (a counter-based
 *          function without state), so the first S' samples of a call are the S'-sample call
 *   ss     R x S x L chars of ( ) . (no terminator)                                       out
 *   E      R x S int32, dcal/mol: drna_score_batch's E(structure) of each sample           out, may be NULL
 *   Epf    R doubles, kcal/mol: the ensemble free energy of the fill the samples come from out, may be NULL
 * A sequence with a bad letter is DRNA_ERR_SEQUENCE, a partition function out of range DRNA_ERR_PF_RANGE, as for
 * drna_ensemble_defect_batch; the outputs are then unspecified.  drna_last_edef_timing afterwards: out[0] = the inside kernel,
 * out[1] = the sample launch, summed over the chunks.  The read-only option "sample_calls" counts the sample launches.
 * A new symbol: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
#define DRNA_SAMPLE_MAX_CHARS (1u << 30)
int drna_sample_structures_batch(drna_engine *e, int R, int L, const char *seqs, int S, const uint64_t *seeds, char *ss,
                                 int32_t *E, double *Epf);

/*
 * Stochastic traceback for two strands: S co-fold structures per sequence pair drawn from the ensemble of drna_cofold_batch and
 * drna_cofold_ensemble_defect_batch.  A structure of the concatenation weighs its Boltzmann factor under the partition
 * function's loop model, times kappa if at least one pair joins the strands (kappa = expDuplexInit, halved when the two strands
 * are the same sequence); the weights sum to exp(-FAB / kT), so p(structure) = weight / exp(-FAB / kT).  For X&X a structure and
 * its rotation by `cut` are two structures, each with the halved weight.  Pairs as for drna_cofold_batch: total length L, both
 * strands concatenated WITHOUT the '&', the first strand `cut` nucleotides long (1 <= cut < L <= max_L).  One inside fill
 * (cofold_pf_kernel, always with its tables in the workspace, whatever "cofold_lds" says), one launch that rebuilds the exterior
 * columns and one sample launch per chunk of workspace slots: R is not limited by max_R.
 *   S      >= 1 samples per pair; R x S x L <= DRNA_SAMPLE_MAX_CHARS, beyond it DRNA_ERR_ARG
 *   seeds  R uint64.  Sample s of pair r depends on the two sequences, seeds[r] and s ALONE, as for drna_sample_structures_batch:
 *          draw k of sample s is u(seeds[r], s, k) of csrc/sample_rng.hpp, k = index of the walk's step
 *   ss     R x S x L chars of ( ) . over the concatenation (no terminator, no '&')          out
 *   E      R x S int32, dcal/mol: drna_cofold_batch's E(structure) of each sample, DuplexInit
 *          included for a connected structure                                                out, may be NULL
 *   F4     R x 4 doubles, kcal/mol: FA, FB, FcAB, FAB of the fill, as drna_cofold_batch        out, may be NULL
 * A pair with a bad letter is DRNA_ERR_SEQUENCE, a partition function out of range DRNA_ERR_PF_RANGE, as for
 * drna_cofold_ensemble_defect_batch; the outputs are then unspecified.  drna_last_edef_timing afterwards: out[0] = the inside
 * kernel, out[1] = the columns and sample launches, summed over the chunks.  The read-only option "cofold_sample_calls" counts the
 * sample launches.  A new symbol: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_cofold_sample_structures_batch(drna_engine *e, int R, int L, int cut, const char *seqs, int S, const uint64_t *seeds,
                                        char *ss, int32_t *E, double *F4);

/*
 * The two structures that represent an ensemble, from its pair probabilities (csrc/fold_mea.hpp; ViennaRNA's fc.MEA(gamma) and
 * fc.centroid()).  P(i,j), 1 <= i < j <= L, is what drna_ensemble_defect_batch (two strands: drna_cofold_ensemble_defect_batch,
 * over the concatenation without '&') returns in bpp -- same values, same layout [i*(L+1)+j].
 *   q(i)       = 1 - sum_j P(min(i,j), max(i,j)), summed in ascending j, not clamped
 *   EA(s)      = sum_{i unpaired in s} q(i) + 2 gamma sum_{(i,j) in s} P(i,j)     for a nested set s of pairs with P > 0
 *   MEA        a maximiser of EA:  M(i,i-1) = 0,
 *              M(i,j) = max( M(i,j-1) + q(j), max_{i <= k < j, P(k,j) > 0} M(i,k-1) + M(k+1,j-1) + 2 gamma P(k,j) ), value M(1,L).
 *              Tie rule: "j unpaired" first, then k ascending; a later candidate replaces only if it is strictly greater.
 *              No hairpin-length or pair-type rule of its own: P > 0 carries both, and for two strands the nick.
 *   centroid   {(i,j) : P(i,j) > 0.5}, always nested; distance = sum_{(i,j) in c} (1 - P(i,j)) + sum_{(i,j) not in c} P(i,j)
 * Arguments:
 *   gamma      > 0 and finite, else DRNA_ERR_ARG
 *   mea_ss     R x L chars of ( ) . (no terminator, no '&')                               out
 *   mea_val    R doubles: EA of mea_ss, M(1,L)                                            out
 *   cen_ss     R x L chars                                                                out
 *   cen_dist   R doubles: expected base-pair distance of the centroid to the ensemble     out
 *   E          R x 2 int32, dcal/mol: drna_score_batch's (two strands: drna_cofold_batch's, DuplexInit included for a connected
 *              structure) E(structure) of mea_ss and of cen_ss                            out, may be NULL
 *   bpp        R*(L+1)*(L+1) doubles: the matrix both structures were read from           out, may be NULL
 * A NULL among seqs, mea_ss, mea_val, cen_ss, cen_dist is DRNA_ERR_ARG.  R is not limited by max_R (chunks of the workspace
 * slots).  The calls need no drna_set_targets() and leave installed targets untouched.  A sequence with a bad letter is
 * DRNA_ERR_SEQUENCE, a partition function out of range DRNA_ERR_PF_RANGE, as for drna_ensemble_defect_batch; the outputs
 * then hold zeros.  Options (drna_set_option / drna_get_option): "mea_lds" (default 1) keeps the table M of sequences of at most
 * "mea_lds_max" (read-only) nucleotides in LDS, 0 puts it into the workspace for every length -- the results are the same bits
 * either way; "mea_calls" (read-only) counts the MEA launches, "mea_candidates" (read-only) the pairs the last call's pruning
 * kept, all sequences.  drna_last_mea_timing: device ms of the last call's inside, outside and MEA launches, summed over its chunks
 * (short inputs take the fused inside + outside launch: out[1] is then ~0).
 * New symbols: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_mea_structures_batch(drna_engine *e, int R, int L, const char *seqs, double gamma, char *mea_ss, double *mea_val,
                              char *cen_ss, double *cen_dist, int32_t *E, double *bpp);
int drna_cofold_mea_structures_batch(drna_engine *e, int R, int L, int cut, const char *seqs, double gamma, char *mea_ss,
                                     double *mea_val, char *cen_ss, double *cen_dist, int32_t *E, double *bpp);
int drna_last_mea_timing(const drna_engine *e, float out[3]);

/*
 * Accessible regions: the partition function with positions held unpaired.  F[r * M + m] (kcal/mol) is the free energy of the
 * ensemble of sequence r in which every position marked by mask m stays unpaired -- RNAfold -p with the hard constraint 'x' on
 * those positions.  The opening energy of the region is Eopen = F[mask] - F[no mask] >= 0 and exp(-Eopen / kT) the probability
 * that the whole region is unpaired.  A masked nucleotide is still that nucleotide next to a pair (mismatches, dangles and the
 * special hairpins see its letter); it just cannot pair.
 *   seqs    R*L chars, row-major, no terminators                                        in
 *   M       masks, >= 1; every sequence is folded under every mask (R*M folds < 2^31)   in
 *   nopair  M*L bytes, row-major, shared by all sequences: non-zero = stays unpaired    in
 *   F       R*M doubles, row-major                                                      out
 * L <= max_L; R and M are not limited by max_R: the R*M folds go through the workspace slots in chunks.  A NULL among seqs,
 * nopair, F or M < 1 is DRNA_ERR_ARG; a bad letter DRNA_ERR_SEQUENCE (the message names the sequence), a partition function
 * out of range DRNA_ERR_PF_RANGE, as for drna_self_dimer_batch.  The call needs no drna_set_targets().  Options
 * (drna_set_option / drna_get_option): "access_lds" (default 1) folds sequences of at most "access_lds_max" (read-only)
 * nucleotides with their tables in LDS, 0 sends every length to the general kernel -- two independent bodies whose results
 * agree within 1e-9 kcal/mol, not bit for bit; "access_lds_calls" (read-only) counts the launches of the LDS kernel.  The host's
 * bound is measured (the LDS kernel loses beyond it); "access_lds" = 2 sends every length the kernel holds,
 * "access_lds_kernel_max" (read-only), to the LDS kernel -- for tests and timing.
 * drna_last_access_timing: device ms of the last call's launches, summed over its chunks.
 * New symbols: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_pf_unpaired_batch(drna_engine *e, int R, int L, const char *seqs, int M, const unsigned char *nopair, double *F);
int drna_last_access_timing(const drna_engine *e, float *ms);

/* device ms summed over the drna_score_batch[_device] calls since the last reset: out[0..3] as drna_last_timing, out[4] = number
 * of calls; out may be NULL (reset only).  Lets a caller time a loop of calls without a query per call. */
int drna_timing_sums(drna_engine *e, double out[5], int reset);

/* device ms of the last drna_ensemble_defect_batch*: out[0] = inside kernel, out[1] = outside kernel; on the fused LDS path
 * out[0] = the one launch, out[1] ~ 0 */
int drna_last_edef_timing(const drna_engine *e, float out[2]);

/*
 * Engine options.  "dual" (default 1): in batches small enough to leave half of the chip idle (4 R <= compute units, L <= 200)
 * the MFE fold of every sequence of at least 170 nt is done by TWO workgroups (fold_mfe_dual.hpp).  Results do not depend
 * on it (integer minima: bit-identical).  0 = always one workgroup per sequence, 2 = two workgroups whenever the batch allows,
 * whatever the length.  DRNA_DUAL in the environment sets the default.
 * "strips" (default 1): sequences of 201 .. 2046 nt are folded by strips of columns, one workgroup per strip of <= 120 columns
 * (fold_pf_strip.hpp, fold_mfe_strip.hpp), in drna_score_batch* and drna_score_ragged.  MFE energies and structures do not
 * depend on it (bit-identical), Epf agrees to 1e-13 kcal/mol (another summation order).  0 = the general one-workgroup kernels,
 * 2 = two strips also for 64 < n <= 200 (diagnostics).  DRNA_STRIPS in the environment sets the default.
 * "pf_helper" (default 1): batches small enough to leave CUs idle (2 R + the MFE fold's workgroups <= CUs, 120 <= n <= 200) fold the
 * partition function with a helper workgroup per sequence that takes the far multiloop split points; Epf is bit-identical either way.
 * "mfe_fark_min_strips" (default 4, i.e. n > 360; one more beside a partition function when there are no pseudoknot rounds):
 * from this many strips on the MFE strips fold their multiloop splits in blocked form (16 x 16 tiles, the far split points as
 * (min,+) tile products); results are identical either way.
 * "mfe_split" (default 2): with pseudoknot rounds the strip path takes a fill launch and a traceback launch per round; a batch of
 * >= 32 sequences then goes in two halves on two streams so that one half's traceback runs under the other's fill; 1 = one part.
 * "cofold_lds" (default 1): drna_cofold_batch and drna_mc_run_cofold fold pairs of at most 64 nt ("cofold_lds_max" reads the bound)
 * with every table in LDS (fold_cofold_lds.hpp); 0 = the general co-fold kernels.  Results are bit-identical either way.
 * "subopt_lds" (default 1): drna_subopt_energy_batch, drna_cofold_subopt_energy_batch and the negative-design step of
 * drna_mc_run_nd / drna_mc_run_cofold_nd fold sequences (pairs: both strands together) of at most "subopt_lds_max" nucleotides
 * (read-only, 79) with their three two-best tables in LDS (fold_subopt_lds.hpp); 0 = the general kernels.  E2 and E12 are
 * bit-identical either way.
 * "edef_lds" (default 1): drna_ensemble_defect_batch[_device], drna_cofold_ensemble_defect_batch and the Edef step of every
 * drna_mc_run* take ONE launch for sequences of at most "edef_lds_max" nucleotides (read-only, 40: up to there the fused kernel is the faster one; its LDS would hold 71) and pairs of at most
 * "cofold_edef_lds_max" nucleotides in all (read-only, 57): inside and outside sweep on tables in LDS (fold_edef_lds.hpp), no
 * workspace slot; 0 = the two launches of the general kernels, which longer inputs take either way.  Two strands: edef and bpp are
 * bit-identical either way.  One strand: the fused kernel sums in another order than outside_kernel, so edef and bpp move in
 * the last bits with the option (about 1e-15; both within 1e-10 of the reference), as Epf does with "strips".  The read-only
 * counter "edef_lds_calls" counts the launches of the fused kernel.
 * "poison" (tests; value = a byte, 0 .. 255): drains the engine's streams, fills every scratch buffer that exists at that moment
 * with the byte (workspaces, result and staging buffers, status words, exchange rows; not the tables, installed targets, motifs
 * or hand-over flags: DESIGN.md 2.1 has the table) and drains again.  No call's results may depend on it.
 */
int drna_set_option(drna_engine *e, const char *name, int value);

/* reads an option back ("dual", "strips"), or the counter "sync_fallbacks": calls in which a fold by several workgroups lost a
 * partner (a bounded wait expired -- HIP promises no dispatch order) and which were therefore redone, transparently, with one
 * workgroup per fold.  Option "strip_fault" = 1 injects such a loss into every strip launch (tests).  "last_workgroups": fold
 * workgroups (partition function + MFE kernels, resident side by side) of the last drna_score_batch call.  "solo_calls_left":
 * after three such calls in a row (a GPU shared with another process) the engine folds with one workgroup per fold for the
 * next 1000 calls, then probes again; setting "dual", "strips" or "pf_helper" ends that at once. */
int drna_get_option(const drna_engine *e, const char *name, int *value);

/* diagnostics (engine created with DRNA_STRIP_DEBUG=1 in the environment): start / end wall clocks (100 MHz ticks) of the MFE
 * strip workgroups of the last launch, out[slot][18][2]; returns the number of sequence slots copied (0 without the buffers) */
int drna_debug_strip_clocks(drna_engine *e, long long *out, int nslots);

/* engine facts: out[0]=device, out[1]=max_R, out[2]=max_L, out[3]=threads per workgroup,
 * out[4]=compute units, out[5]=bytes of device workspace */
int drna_info(const drna_engine *e, int64_t out[6]);

/*
 * Host-side pieces of the Monte-Carlo inner loop, batched over replicas (plain CPU code, no engine needed).
 *
 * drna_simscore_batch: SimScore(ref, query) of utils/sim_score.py:62-147 for R query structures against one
 * reference; outputs are the reference's rounded mcc / recall / precision (NOT 1 - x).  '&' must already be
 * replaced by "Ee" as utils/energy_scores.py:79 does.
 */
int drna_simscore_batch(int R, int L, const char *ref, const char *queries, double *mcc, double *recall,
                        double *precision);

/*
 * Sequence motifs (-motifs KEY,VALUE,KEY,VALUE,...; DesiRNA.py:212-224, score_motifs of utils/sequence_utils.py:1231-1251): a
 * motif that occurs anywhere in a sequence adds its value to the sequence's score, once however often it occurs; the term of
 * a sequence is 0 + the values of the motifs that occur, in the order given, and it is the last addition to the score (after
 * the -sf sum, the alternative-structure term, the negative-design term and the oligomer / monomer-fraction bonus,
 * utils/energy_scores.py:121-123).  A motif is a string over A C G T U W S M K R Y B D H V N: W = AU, S = GC, M = AC, K = GU,
 * R = AG, Y = CU, B = CGU, D = AGU, H = ACU, V = ACG, N = ACGU; A C G U T match themselves only (N does not match T).  Any other
 * character of a sequence matches nothing: a two-strand string is searched with its '&' in place, so no motif matches across
 * the nick.  The empty motif occurs in every sequence.  Motifs of at most 64 letters are searched bit-parallel (one pass over
 * the sequence per motif, ended by the first hit), longer ones by a window scan.
 *   n_motifs    >= 0
 *   motif_len   n_motifs ints, each >= 0
 *   motifs      the motifs' letters, concatenated (sum of motif_len chars, no terminator needed)
 *   value       n_motifs doubles
 * A letter outside the sixteen above (lower case included) is DRNA_ERR_ARG.
 *
 * drna_motif_score_batch (no engine needed): out[r] = the term of sequence r of R sequences of L >= 1 chars; n_motifs == 0
 * writes zeros.
 *
 * drna_set_motifs: the motif set of the ENGINE, which every drna_mc_run* loop (drna_mc_run, _nd, _oa, _cofold, _cofold_nd,
 * _ragged, _ragged_nd) adds to the score of every proposal -- the term of the chain's own string, two strands with the '&', the
 * same set for every puzzle of a ragged loop.  n_motifs == 0 clears the set; a loop with an empty set does no work for it and
 * returns what it returned before the set existed.  The set stays until the next call: a caller that shares an engine between
 * runs sets it (or clears it) before each run.  On DRNA_ERR_ARG the engine's set is unchanged.  The read-only option "motifs"
 * (drna_get_option) is the number of motifs set.
 * New symbols: no existing signature or buffer changes, DRNA_ABI_VERSION stays 3.
 */
int drna_motif_score_batch(int R, int L, const char *seqs, int n_motifs, const int32_t *motif_len, const char *motifs,
                           const double *value, double *out);
int drna_set_motifs(drna_engine *e, int n_motifs, const int32_t *motif_len, const char *motifs, const double *value);

/*
 * Per-replica random streams of the host helpers: the reference's worker calls random.seed(replica_index) at the start of
 * every exchange step (utils/replica_exchange_monte_carlo.py:227-228 with seeds = [0 .. R-1], :250) and then draws from
 * Python's global Mersenne Twister.  drna_rng_seed(seeds) = random.seed(int) for each of R streams (MT19937 init_by_array
 * on the integer's 32-bit digits); drna_rng_random = one random.random() per stream (53-bit, two outputs).
 *   rng_state   R * DRNA_RNG_WORDS uint32 (624 state words + position), owned by the caller
 */
#define DRNA_RNG_WORDS 625
int drna_rng_seed(int R, const uint64_t *seeds, uint32_t *rng_state);
int drna_rng_random(int R, uint32_t *rng_state, double *out);

/*
 * drna_propose_batch: one proposal per replica, the move set of mutate_sequence / get_mutation_position /
 * expand_cases (utils/sequence_utils.py:926-1136) for single-chain targets without alternative structures.
 *   target        L chars, every bracket family is a design pair
 *   allowed_mask  L bytes, bit0 A, bit1 C, bit2 G, bit3 U: letters_allowed of get_nt_list (:454-525)
 *   seqs, mfe_ss  R*L chars: current sequence and current MFE structure of each replica
 *   shelf_index   R ints: index of the replica's temperature shelf; the targeted-mutation probability is
 *                 round(linspace(tm_max, tm_min, n_shelves)[index], 2) (:963-967)
 *   rng_state     R * DRNA_RNG_WORDS uint32: one MT19937 stream per replica (drna_rng_seed), advanced in place; the
 *                 draws are CPython's (random(), choice(), choices()), in the order of the reference's code
 *   out_seqs      R*L chars
 */
int drna_propose_batch(int R, int L, const char *target, const unsigned char *allowed_mask, const char *seqs,
                       const char *mfe_ss, const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min,
                       int targeted, uint32_t *rng_state, char *out_seqs);

/*
 * drna_propose_batch_alt: the same move set for targets WITH alternative structures (>alt_sec_struct): positions that sit
 * in a "snake" (a connected component of the pair graph of target + alternative structures, utils/sequence_utils.py:143-388)
 * move the whole component to another of its Watson-Crick colourings (:1081-1095); alternative pairs outside snakes are
 * ordinary design pairs.
 *   partner        L int32: partner of every design pair (target pairs + ordinary alternative pairs), -1 = none
 *   snake_of       L int32: snake index of a position or -1 (may be NULL when n_snakes == 0)
 *   snake_off      n_snakes+1 int32: snake k owns snake_nodes[snake_off[k] .. snake_off[k+1])  (ascending positions)
 *   snake_nstates  n_snakes int32 (1..4); snake_states: for snake k, 4 slots of len_k letters at 4*snake_off[k]
 * False negatives / positives of the targeted-mutation rule are taken against `target` only (input_file.target_pairs_tupl).
 */
int drna_propose_batch_alt(int R, int L, const char *target, const int32_t *partner, const unsigned char *allowed_mask,
                           const int32_t *snake_of, int n_snakes, const int32_t *snake_off, const int32_t *snake_nodes,
                           const int32_t *snake_nstates, const char *snake_states, const char *seqs, const char *mfe_ss,
                           const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                           uint32_t *rng_state, char *out_seqs);

/*
 * drna_metropolis_batch: mc_delta of utils/replica_exchange_monte_carlo.py:26-57 for R replicas: accept iff
 * score_m <= score_o, else with probability exp(-Lconst / T * (score_m - score_o)) (one draw, only then).
 */
int drna_metropolis_batch(int R, const double *score_o, const double *score_m, const double *temps, double Lconst,
                          uint32_t *rng_state, unsigned char *accept, unsigned char *better);

/*
 * drna_mc_run: n_iter Monte-Carlo iterations of ALL replicas without returning to the caller -- the body of
 * single_replica_design (utils/replica_exchange_monte_carlo.py:176-210) for R replicas in lock-step: proposal
 * (drna_propose_batch[_alt] rules; partner / snake arrays may be NULL / 0 for plain targets), scoring of the R proposals on the
 * GPU (drna_score_batch with flags | PF | MFE | EVAL against the structures of drna_set_targets), SimScore, the -sf sum
 * (term_id: 0 Ed-Epf, 1 1-MCC, 2 sln_Epf, 3 Ed-MFE, 4 1-precision, 5 1-recall, 6 Edef; weights term_w; + mean E(alt) - Epf when
 * alternative structures are installed), Metropolis acceptance, state update.
 *   in/out per replica: seqs, mfe_ss (R*L chars), score, mcc1 (= 1 - MCC), Epf, Ed (kcal/mol), rng_state
 *   counters[3] += accepted, accepted-better, rejected;  best[4] = {1-MCC, score, Epf, Ed} and best_seq / best_ss (L chars)
 *   are replaced whenever an accepted state is better (lower 1-MCC, then lower score)
 */
int drna_mc_run(drna_engine *e, int R, int L, int n_iter, const char *target, const int32_t *partner,
                const unsigned char *allowed_mask, const int32_t *snake_of, int n_snakes, const int32_t *snake_off,
                const int32_t *snake_nodes, const int32_t *snake_nstates, const char *snake_states,
                const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted, const double *temps,
                double Lconst, int n_terms, const int32_t *term_id, const double *term_w, uint32_t flags,
                uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed,
                int64_t *counters, char *best_seq, char *best_ss, double *best);

/*
 * Two strands.  drna_propose_batch_co: the move set of drna_propose_batch for targets that contain one '&' (the reference's
 * hetero-dimer and homodimer modes).  Every string (target, seqs, mfe_ss, out_seqs; L chars) keeps the '&' at the target's
 * column as a fixed, unpaired letter: positions, the +-3 window and its bounds and the draw counts include it, and a targeted
 * move that lands on it (or on another fixed position) changes nothing after the same draws.  allowed_mask of the '&' column is 0.
 *   oligo_state   1 hetero-dimer, 2 homodimer: the reference's strand-copy rules follow every move (utils/sequence_utils.py:
 *                 1104-1126): two equal sub-structures -- the strand that changed is copied over the other; two different ones --
 *                 the two ends of a pair move are crossed over between the strands
 */
int drna_propose_batch_co(int R, int L, const char *target, const unsigned char *allowed_mask, int oligo_state,
                          const char *seqs, const char *mfe_ss, const int32_t *shelf_index, int n_shelves, double tm_max,
                          double tm_min, int targeted, uint32_t *rng_state, char *out_seqs);

/*
 * drna_mc_run_cofold: drna_mc_run for a two-strand target.  L = nucleotides of both strands, cut = length of the first; the
 * state strings (target, seqs, mfe_ss, best_seq, best_ss) have L + 1 chars with the '&' at column cut; drna_set_targets holds
 * the target without it.  Scoring step of the reference's two-strand branch (utils/energy_scores.py:70-118): co-fold MFE +
 * traceback, partition function and two-strand evaluation of the R proposals (pairs of at most 64 nt with their tables in LDS,
 * option "cofold_lds"); Epf = FAB; SimScore with the '&' -> "Ee" substitution; the -sf terms of drna_mc_run (Ed-MFE against the
 * co-fold MFE, Edef in the co-fold ensemble); oligo_fraction from FA, FB, FcAB; then -kT ln(oligo_fraction) for a hetero-dimer or
 * a homodimer of two different sub-structures, -kT ln(1 - oligo_fraction) for two equal ones, added after the -sf sum.
 *   in/out per replica: as drna_mc_run, and oligo_frac, bonus (R doubles)
 *   best[6] = {1-MCC, score, Epf, Ed, oligo_fraction, bonus}
 */
int drna_mc_run_cofold(drna_engine *e, int R, int L, int cut, int n_iter, const char *target, const unsigned char *allowed_mask,
                       int oligo_state, const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                       const double *temps, double Lconst, int n_terms, const int32_t *term_id, const double *term_w,
                       uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed,
                       double *oligo_frac, double *bonus, int64_t *counters, char *best_seq, char *best_ss, double *best);

/*
 * Negative design (-nd on; utils/energy_scores.py:104-108) in the native loops.  drna_mc_run_nd and drna_mc_run_cofold_nd are
 * drna_mc_run and drna_mc_run_cofold with one more step between the scoring of the R proposals and the Metropolis test: the
 * proposals whose 1 - MCC is exactly 0 (H of them) get their second-best fold in one launch of H workgroups (drna_subopt_energy_batch
 * / drna_cofold_subopt_energy_batch rules, option "subopt_lds") and lose E2 / 100 - Epf.  H = 0 launches nothing.  Order of
 * additions: the -sf sum, the alternative-structure term, the negative-design term and, for two strands, only then the oligomer /
 * monomer-fraction bonus.  The random draws are those of the plain entry points, so a run in which no proposal is ever solved
 * returns the same arrays bit for bit.
 *   subopt_e   R doubles, in/out, kcal/mol: the second-best energy that belongs to each replica's current state (0 where that
 *              state is unsolved or no second structure lies within 49 kcal/mol); travels with an accepted state.  NULL is
 *              DRNA_ERR_ARG
 *   best       one value more than in the plain entry point: best[4] (two strands: best[6]) = subopt_e of the best state
 * New symbols: no existing signature changes, DRNA_ABI_VERSION stays 3.
 */
int drna_mc_run_nd(drna_engine *e, int R, int L, int n_iter, const char *target, const int32_t *partner,
                   const unsigned char *allowed_mask, const int32_t *snake_of, int n_snakes, const int32_t *snake_off,
                   const int32_t *snake_nodes, const int32_t *snake_nstates, const char *snake_states,
                   const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted, const double *temps,
                   double Lconst, int n_terms, const int32_t *term_id, const double *term_w, uint32_t flags,
                   uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed,
                   int64_t *counters, char *best_seq, char *best_ss, double *best, double *subopt_e);
int drna_mc_run_cofold_nd(drna_engine *e, int R, int L, int cut, int n_iter, const char *target, const unsigned char *allowed_mask,
                          int oligo_state, const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                          const double *temps, double Lconst, int n_terms, const int32_t *term_id, const double *term_w,
                          uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed,
                          double *oligo_frac, double *bonus, int64_t *counters, char *best_seq, char *best_ss, double *best,
                          double *subopt_e);

/*
 * Avoid oligomerization (-oa on = the reference's -o on, oligo_state "avoid"; utils/energy_scores.py:118-119, :412-419).
 *
 * drna_self_dimer_batch: the partition function of every sequence folded against a copy of itself (s & s), replacing
 * RNA.fold_compound(s + "&" + s).pf_dimer() and dimer_multichain_energy.oligo_fraction (:36-50).  seqs: R x L letters.
 * F4[r] = {FA, FB (the same strand again), FcAA, FAA} in kcal/mol, in drna_cofold_batch's layout and with its values for
 * (s + s, cut = L) -- the symmetry factor of two equal strands included; oligo_frac (R doubles, may be NULL) = the fraction of
 * strands bound in the dimer at 1 mM.  L <= max_L: the engine is sized for L, not 2 L (fold_self_dimer.hpp stores ~1.5 L^2 cells,
 * which fit the partition function's workspace slot of an L-nt sequence; nothing is allocated).  R is not limited by max_R: a
 * larger batch goes through the workspace slots in chunks.  Sequences of at most "self_dimer_lds_max" nucleotides (read-only
 * option, 62) keep every table in LDS; option "self_dimer_lds" (default 1) = 0 sends every length to the workspace kernel.
 * Results are bit-identical either way.
 *
 * drna_mc_run_oa: drna_mc_run (subopt_e NULL) or drna_mc_run_nd (subopt_e given) with one more step: after the score batch of
 * the R proposals has drained, all R proposals get their self-dimer partition function in one launch of R workgroups;
 * oligo_fraction from it, and -kT ln(1 - oligo_fraction) is the LAST addition to the score, after the negative-design term
 * (the reference's order, :104-119).  The random draws are those of drna_mc_run.
 *   oligo_frac, bonus   R doubles, in/out: the values that belong to each replica's current state; travel with an accepted state
 *   best                the two-strand layout: {1-MCC, score, Epf, Ed, oligo_fraction, bonus[, subopt_e]}
 * New symbols: no existing signature changes, DRNA_ABI_VERSION stays 3.
 */
int drna_self_dimer_batch(drna_engine *e, int R, int L, const char *seqs, double *F4, double *oligo_frac);
int drna_mc_run_oa(drna_engine *e, int R, int L, int n_iter, const char *target, const int32_t *partner,
                   const unsigned char *allowed_mask, const int32_t *snake_of, int n_snakes, const int32_t *snake_off,
                   const int32_t *snake_nodes, const int32_t *snake_nstates, const char *snake_states,
                   const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted, const double *temps,
                   double Lconst, int n_terms, const int32_t *term_id, const double *term_w, uint32_t flags,
                   uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed,
                   int64_t *counters, char *best_seq, char *best_ss, double *best, double *subopt_e, double *oligo_frac,
                   double *bonus);

/*
 * drna_mc_run_ragged: drna_mc_run for a SET of P design problems of different lengths (BASELINE config 4 as a design run),
 * all advanced together for n_iter iterations: per iteration one proposal per chain, ONE ragged scoring of all chains
 * (drna_score_ragged rules: sequences of every length side by side, one workgroup per fold or strips above 200 nt), then the
 * Metropolis draws in chain order.  Per chain the draws, scores and results are those of drna_mc_run on that puzzle alone;
 * the pace is that of the longest puzzle in the call.
 * Chains are ordered puzzle after puzzle: puzzle p owns R_of[p] chains of L_of[p] letters, C = sum R_of[p] chains in all.
 *   per puzzle   targets, allowed_mask: concatenated, sum L_of[p] chars / bytes;  n_shelves: P ints;
 *                counters: 3 per puzzle;  best_seq, best_ss: concatenated like the targets;  best: 4 per puzzle
 *   per chain    shelf_index, temps, score, mcc1, Epf, Ed: C values;  rng_state: C * DRNA_RNG_WORDS;
 *                seqs, mfe_ss: concatenated chain after chain (sum R_of[p] * L_of[p] chars)
 *   shared       n_iter, tm_max, tm_min, targeted, Lconst, the -sf terms and weights, flags: as in drna_mc_run
 * The call installs the P targets itself, as drna_set_targets_ragged(e, P, L_of, targets) does: it REPLACES the engine's ragged
 * target set (a caller that scores with drna_score_ragged afterwards installs its own set again).  The set of puzzles usually
 * shrinks from call to call of a run, and a set left from an earlier call would be evaluated against the wrong structures.
 * Scope: one strand and the plain brackets ( ) . only (a target with '&' or another bracket family is DRNA_ERR_ARG); no
 * alternative structures, no negative-design and no self-dimer step; -sf terms 0 .. 5, sln_Epf with the chain's own length
 * (term 6, Edef, is DRNA_ERR_ARG).  Limits, as for drna_score_ragged: C <= max_R and sum R_of[p] * L_of[p] <= max_R * max_L.
 * A new symbol: no existing signature changes, DRNA_ABI_VERSION stays 3.
 */
int drna_mc_run_ragged(drna_engine *e, int P, const int32_t *R_of, const int32_t *L_of, int n_iter, const char *targets,
                       const unsigned char *allowed_mask, const int32_t *shelf_index, const int32_t *n_shelves, double tm_max,
                       double tm_min, int targeted, const double *temps, double Lconst, int n_terms, const int32_t *term_id,
                       const double *term_w, uint32_t flags, uint32_t *rng_state, char *seqs, char *mfe_ss, double *score,
                       double *mcc1, double *Epf, double *Ed, int64_t *counters, char *best_seq, char *best_ss, double *best);

/*
 * The auxiliary folds of a ragged batch, and the lock-step loop with them.  New symbols; DRNA_ABI_VERSION stays 3.
 *
 * drna_ensemble_defect_ragged: the ensemble defect (ScoreSeq.get_ensemble_defect, utils/energy_scores.py:362-374) of R sequences of
 * lengths lens[r], concatenated, each against structure target_of[r] of drna_set_targets_ragged.  Argument rules of
 * drna_score_ragged (R <= max_R, lengths within max_L, target_of[r] names a structure of the sequence's length, sum of lengths
 * <= max_R * max_L).  Per sequence the value is drna_ensemble_defect_batch's for that length, bit for bit: with option
 * "edef_lds" the sequences of at most 40 nt share ONE launch of the fused LDS kernel (counted in "edef_lds_calls"), the others
 * go through pf_kernel + outside_kernel in chunks of the workspace slots.  No pair probabilities.  drna_last_edef_timing is the
 * sum over the launches.  A failed sequence is named by the caller's index r.
 *
 * drna_subopt_energy_ragged: the second-best energy (get_first_suboptimal_structure_and_energy(seq, fc, 1)[1],
 * utils/energy_scores.py:104-108) of R sequences of lengths lens[r], concatenated.  E2 / E12 as drna_subopt_energy_batch returns
 * them for each length (E12 may be NULL); with option "subopt_lds" the sequences of at most 79 nt fold in LDS.  R <= max_R and
 * R <= workspace slots, as for drna_subopt_energy_batch.
 *
 * drna_mc_run_ragged_nd: drna_mc_run_ragged with what drna_mc_run_nd adds to drna_mc_run.  -sf term 6 (Edef) is accepted: every
 * iteration adds one ragged ensemble-defect pass over all chains.  subopt_e (C doubles, one per chain; NULL: no negative design):
 * the solved proposals of an iteration (utils/energy_scores.py:93-94,104-108), whatever their puzzles, get their second-best
 * folds in one ragged launch set; subopt_e[r] is the second-best energy of chain r's state (0 where unsolved) and best holds
 * 5 values per puzzle (best[4] = that of the best state); needs C <= workspace slots.  Per chain the draws, scores and results
 * are those of drna_mc_run_nd on that puzzle alone.  Everything else as in drna_mc_run_ragged.
 */
int drna_ensemble_defect_ragged(drna_engine *e, int R, const int32_t *lens, const char *seqs, const int32_t *target_of,
                                double *edef);
int drna_subopt_energy_ragged(drna_engine *e, int R, const int32_t *lens, const char *seqs, int32_t *E2, int32_t *E12);
int drna_mc_run_ragged_nd(drna_engine *e, int P, const int32_t *R_of, const int32_t *L_of, int n_iter, const char *targets,
                          const unsigned char *allowed_mask, const int32_t *shelf_index, const int32_t *n_shelves, double tm_max,
                          double tm_min, int targeted, const double *temps, double Lconst, int n_terms, const int32_t *term_id,
                          const double *term_w, uint32_t flags, uint32_t *rng_state, char *seqs, char *mfe_ss, double *score,
                          double *mcc1, double *Epf, double *Ed, int64_t *counters, char *best_seq, char *best_ss, double *best,
                          double *subopt_e);

#ifdef __cplusplus
}
#endif
#endif
