// engine.hip -- host side of the gfx950 replica-scoring engine and its C ABI (include/desirna_amd.h).
//
// One engine = one GPU.  Per call the three kernel families run concurrently on their own HIP
// streams (MFE fill+traceback, partition function, structure evaluation: they are independent per
// sequence, reference utils/energy_scores.py:150-151,75), bracketed by HIP events so bench.py can
// read per-kernel device times without a profiler.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/desirna_amd.h"
#include "eval_structure.hpp"
#include "fold_mfe.hpp"
#include "fold_cofold.hpp"
#include "fold_cofold_lds.hpp"
#include "fold_self_dimer.hpp"
#include "fold_mfe_lds.hpp"
#include "fold_mfe_dual.hpp"
#include "fold_fused.hpp"
#include "fold_mfe_strip.hpp"
#include "fold_outside.hpp"
#include "fold_pf.hpp"
#include "fold_pf_lds.hpp"
#include "fold_pf_strip.hpp"
#include "fold_sample.hpp"
#include "fold_cofold_sample.hpp"
#include "fold_mea.hpp"
#include "fold_subopt.hpp"
#include "fold_cofold_subopt.hpp"
#include "fold_subopt_lds.hpp"
#include "fold_cofold_outside.hpp"
#include "fold_edef_lds.hpp"
#include "fold_access.hpp"
#include "host_driver.hpp"
#include "tables.hpp"

using namespace drna;

static std::string g_create_error;

#ifndef DRNA_MFE_FARK_MIN_STRIPS
#define DRNA_MFE_FARK_MIN_STRIPS 4
#endif
constexpr int MFE_FARK_MIN_STRIPS = DRNA_MFE_FARK_MIN_STRIPS;   // (measured against prebuilt variants)
// hand-over flags hold (epoch << 12 | diagonal) for the strips and ((epoch * 8 + round) << 10 | diagonal) for the two-workgroup
// kernel, compared wrap-safe: valid while live values are less than 2^31 apart, i.e. 2^19 (2^18) epochs.  Reset at a quarter of that.
constexpr int STRIP_EPOCH_RESET = 1 << 17, DUAL_EPOCH_RESET = 1 << 16;
// one set of hand-over flags of a multi-workgroup fold: ints flags on the device, zero when allocated; the epoch grows by one per
// launch (strips) or call, and flags and epoch go back to zero at reset_at (flags_ready)
struct EpochFlags { int* d = nullptr; size_t ints = 0; int epoch = 0; int reset_at = 0; };
struct drna_engine {
  int device = 0, max_R = 0, max_L = 0, cus = 0;
  HostTables H;
  MfeTables* d_mfeT = nullptr;
  PfTables* d_pfT = nullptr;
  Plan* d_plan = nullptr;
  int *d_hp_len = nullptr, *d_bulge_len = nullptr, *d_int_len = nullptr;
  double *d_hp_w = nullptr, *d_scale = nullptr, *d_eMLb = nullptr;
  int32_t* d_ws_mfe = nullptr;
  double* d_ws_pf = nullptr;
  size_t ws_bytes = 0;
  int ws_slots = 0;               // sequences the fold workspaces hold at once: max_R, or fewer under the workspace budget (DRNA_WS_GB,
                                  // default 8): larger batches are folded in chunks of ws_slots, back to back on the same streams
  // device copies of the sequences and results of the ragged, ensemble-defect, second-best and co-fold entry points
  char* d_seqs = nullptr;
  double* d_Epf = nullptr;
  int32_t* d_Emfe = nullptr;
  char* d_ss = nullptr;
  int32_t* d_Ed = nullptr;
  // per-sequence status words, host-mapped so no copy is needed after the streams drain
  int32_t *h_status = nullptr, *d_status = nullptr;   // [0,R) mfe, [max_R, max_R+R) pf
  short* d_pt = nullptr;
  int n_targets = 0, L_targets = 0;
  hipStream_t s_mfe = nullptr, s_pf = nullptr, s_eval = nullptr;
  hipEvent_t ev_mfe2 = nullptr;                // the second half of a batch whose MFE fold takes several launches runs on s_eval (no stream of
                                               // its own: the runtime maps streams onto a few hardware queues, and streams that share one serialize)
  hipEvent_t ev_start = nullptr, ev_end = nullptr, ev_m0 = nullptr, ev_m1 = nullptr, ev_p0 = nullptr,
             ev_p1 = nullptr, ev_e0 = nullptr, ev_e1 = nullptr;
  float timing[4] = {0, 0, 0, 0};
  double timing_sum[5] = {0, 0, 0, 0, 0};     // mfe, pf, eval, total ms summed over drna_score_batch_device calls; [4] = calls
  // ensemble defect (outside recursion): workspace allocated on first use
  double* d_ws_out = nullptr;
  double* d_edef = nullptr;
  hipEvent_t ev_o0 = nullptr, ev_o1 = nullptr, ev_o2 = nullptr;
  hipEvent_t ev_gate = nullptr;                // the partition function's launch waits for it (see pf_gate_round)
  float timing_edef[2] = {0, 0};
  // stochastic traceback (fold_sample.hpp): the q5 columns of ws_slots sequences, allocated on first use
  double* d_q5s = nullptr;
  int sample_calls = 0;     // launches of sample_kernel (read-only option "sample_calls")
  // ... for two strands (fold_cofold_sample.hpp): the columns q5, qA3, qB5, q5c of ws_slots pairs, allocated on first use
  double* d_cocols = nullptr;
  int cofold_sample_calls = 0;   // launches of cofold_sample_kernel (read-only option "cofold_sample_calls")
  // MEA and centroid structures (fold_mea.hpp): an all-unpaired pair table for the outside pass in front of them, allocated on first use
  short* d_mea_pt = nullptr;
  bool mea_lds = true;      // option "mea_lds": sequences of at most MEA_LDS_MAX nt keep the table M in LDS
  int mea_calls = 0;        // launches of mea_kernel (read-only option "mea_calls")
  int mea_cands = 0;        // candidate pairs the pruning left in the last call, all sequences (read-only option "mea_candidates")
  float timing_mea[3] = {0, 0, 0};
  // ragged batches: per-sequence descriptors (len, off, target, two index lists) and the structures' pair tables.  Three blocks
  // of 7 max_R ints (rg_block): a lock-step loop keeps its scoring plan, its ensemble-defect plan and the second-best fold's
  // lists on the device side by side
  int* d_rg = nullptr;
  short* d_rpt = nullptr;
  int* d_rpt_off = nullptr;
  std::vector<int> rt_len;
  double* d_F4 = nullptr;   // co-fold free energies (FA, FB, FcAB, FAB per pair)
  double *hm_F4 = nullptr, *dm_F4 = nullptr;   // ... of drna_cofold_batch and drna_mc_run_cofold: host-mapped like hm_Epf, allocated on first use
  bool cofold_lds = true;   // option "cofold_lds": pairs of at most CO_LDS_MAX nt fold with their tables in LDS (fold_cofold_lds.hpp)
  bool self_dimer_lds = true;   // option "self_dimer_lds": self-dimers of at most SD_LDS_MAX nt keep their tables in LDS (fold_self_dimer.hpp)
  bool edef_lds = true;     // option "edef_lds": ensemble defects of at most EDEF_LDS_HOST_MAX nt (pairs: CO_EDEF_LDS_MAX) in one launch, tables in LDS (fold_edef_lds.hpp)
  int edef_lds_calls = 0;   // launches of that kernel (read-only option "edef_lds_calls")
  // partition function with positions held unpaired (fold_access.hpp): the masks of the last call on the device, grown on demand
  unsigned char* d_nopair = nullptr;
  size_t nopair_cap = 0;
  bool access_lds = true;   // option "access_lds": sequences of at most ACCESS_LDS_HOST_MAX nt keep their tables in LDS (access_lds_kernel)
  bool access_lds_force = false;   // option "access_lds" = 2: up to the kernel's own ACCESS_LDS_MAX (tests, the timing tool)
  int access_lds_calls = 0; // launches of that kernel (read-only option "access_lds_calls")
  float timing_access = 0;  // device time of the last drna_pf_unpaired_batch call, its chunks summed (drna_last_access_timing)
  bool subopt_lds = true;   // option "subopt_lds": second-best folds of at most SUB_LDS_MAX nt keep their tables in LDS (fold_subopt_lds.hpp)
  // K-best structures: workspace for kb_chunk sequences, allocated on first use
  int32_t* d_ws_kb = nullptr;
  int32_t* d_kbE = nullptr;
  char* d_kbss = nullptr;
  int kb_chunk = 0;
  // host-mapped staging of the host-buffer entry point: the kernels read the sequences from and write their results to
  // pinned host memory directly, so a batch costs no hipMemcpy round trips (12.8 KB in, 13.6 KB out at R=64, L=200)
  char *hm_seqs = nullptr, *hm_ss = nullptr, *dm_seqs = nullptr, *dm_ss = nullptr;
  double *hm_Epf = nullptr, *dm_Epf = nullptr;
  int32_t *hm_Emfe = nullptr, *dm_Emfe = nullptr, *hm_Ed = nullptr, *dm_Ed = nullptr;
  size_t hm_Ed_cap = 0;
  // two-workgroup kernels (small batches: 4 R <= CUs, n <= 200): exchange rows and flags, allocated on first use
  bool dual = true;               // DRNA_DUAL=0 turns them off
  bool dual_force = false;        // option "dual" = 2: also beside a partition function (tests, diagnostics)
  int dual_cap = 0;               // sequences the exchange buffers hold
  EpochFlags dflags{nullptr, 0, 0, DUAL_EPOCH_RESET};     // [2 kernels][R][64], grows with the batch (fold_common.hpp, DualLink)
  int32_t *d_xs = nullptr, *d_xa_mfe = nullptr, *d_xb_mfe = nullptr;
  // strip kernels (fold_pf_strip.hpp: 200 < n <= 2046, several workgroups per sequence): one flag line per (sequence, strip)
  int strips = 1;                 // 0 off (general kernel), 1 for n > 200, 2 also for 64 < n <= 200 (two strips; diagnostics)
  int flag_resets = 0;            // times the hand-over flags were zeroed because an epoch neared the compare range
  int strip_fault = 0;            // option "strip_fault": inject a lost strip (tests)
  bool cur_with_pf = false;       // the call being enqueued also folds the partition function
  int mfe_fark_min_strips = MFE_FARK_MIN_STRIPS;   // option "mfe_fark_min_strips": MFE strips fold in blocked form from this many strips on
  int mfe_split = 2;              // option "mfe_split": parts of a batch (on two streams) for the pseudoknot rounds of the strip path; 1 = off
  bool helper_fault = false;      // tests: the helper workgroups of the partition function leave at once (a lost partner)
  bool pf_helper = true;          // small batches: a helper workgroup per sequence computes the far multiloop split points of the
                                  // partition function (fold_pf_lds.hpp, pf_kfar_helper); option "pf_helper"
  EpochFlags pflags{nullptr, 0, 0, STRIP_EPOCH_RESET};    // its hand-over flags: per sequence two 128-byte lines, grows with the batch
  bool fused = true;              // small batches: both folds in ONE launch of 4 R workgroups (fold_fused.hpp); option "fused", DRNA_FUSED=0 turns it off.
                                  // On since the end of round 4: 0.413 against 0.420 ms of device time at R = 64 x L = 200 (the two launches' kernels
                                  // start and end a few us apart; the host pays the same 14 us either way)
  int fused_blocks_per_cu = -1;   // occupancy query of the fused kernel (-1: not asked yet)
  int pair_blocks_per_cu = -1;    // ... of the two-workgroup MFE kernel and the partition function with helpers (the smaller of the two answers)
  long long *h_clk = nullptr, *d_clk = nullptr;   // host-mapped: start / end wall clock of every block of the fused launch
  int clk_cap = 0;
  bool last_fused = false;        // the last drna_score_batch_device call went through the fused launch
  int last_wgs = 0;               // fold workgroups of the last drna_score_batch call (partition function + MFE kernels, resident side by side)
  int sync_fallbacks = 0;         // calls that lost a multi-workgroup fold (ST_SYNC) and were redone with one workgroup per fold
  // A GPU shared with another process (or a runtime that stops dispatching in block order) loses partners call after call, and
  // every lost call costs its wait budget before it is redone.  Three fallbacks in a row switch the multi-workgroup paths off
  // for the next SOLO_CALLS calls (option "solo_calls_left"); then one call probes again.  Any set_option of the paths resets it.
  int fallback_streak = 0, solo_left = 0;
  bool in_fallback = false;
  EpochFlags sflags{nullptr, 0, 0, STRIP_EPOCH_RESET};    // [2: partition function, MFE][max_R][STRIP_MAXS][32]; both halves share the epoch
  int32_t* d_srec = nullptr;      // MFE strips: exchange records and list counts, srec_stride int32 per sequence
  long long srec_stride = 0;
  long long* d_sclk = nullptr;    // DRNA_STRIP_DEBUG=1: start / end clocks of the MFE strip workgroups of the last launch
  int* d_sdbg = nullptr;          // DRNA_STRIP_DEBUG=1: [2][max_R][8] words written by a strip whose wait failed
  std::string err; drna_host::MotifSet motifs;   // motifs (drna_set_motifs): what every drna_mc_run* loop adds to its proposals' scores; empty: none
};

#define HIP_TRY(call)                                                                      \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess) {                                                                \
      e->err = std::string(#call) + ": " + hipGetErrorString(_e);                          \
      /* kernels of this call may already be enqueued on the engine's other streams: the next call assumes idle   */ \
      /* streams (it rewrites h_status and the workspaces), so drain the device before handing the error back     */ \
      (void)hipDeviceSynchronize();                                                        \
      return DRNA_ERR_DEVICE;                                                              \
    }                                                                                      \
  } while (0)

template <typename T>
static hipError_t upload(T** dst, const T* src, size_t count) {
  hipError_t r = hipMalloc((void**)dst, count * sizeof(T));
  if (r != hipSuccess) return r;
  return hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice);
}

static size_t mfe_ws_stride(int ld) { return (size_t)5 * ld * ld; }                       // int32
static size_t pf_ws_stride(int ld) { return (size_t)7 * ld * ld + ((size_t)ld * ld + 7) / 8; }  // doubles

// kernel arguments of a batch of sequences seqs (L = 0 for a ragged batch) with tables of pitch ld in the engine's workspaces;
// call sites add what is their own (ragged descriptors, workspace offset of a chunk, helper flags, q5out, the strands' cut)
static MfeArgs mfe_args(const drna_engine* e, const char* seqs, int L, int ld, int pk_rounds, int32_t* Emfe, char* ss) {
  MfeArgs a;
  a.T = e->d_mfeT; a.plan = e->d_plan; a.hp_len = e->d_hp_len; a.seqs = seqs; a.L = L; a.ld = ld;
  a.pk_rounds = pk_rounds;
  a.ws = e->d_ws_mfe; a.ws_stride = (long long)mfe_ws_stride(ld);
  a.Emfe = Emfe; a.ss = ss; a.status = e->d_status;
  return a;
}
static PfArgs pf_args(const drna_engine* e, const char* seqs, int L, int ld, double* Epf) {
  PfArgs a;
  a.T = e->d_pfT; a.plan = e->d_plan; a.hp_w = e->d_hp_w; a.scale = e->d_scale; a.eMLb = e->d_eMLb;
  a.seqs = seqs; a.L = L; a.ld = ld;
  a.ws = e->d_ws_pf; a.ws_stride = (long long)pf_ws_stride(ld);
  a.Epf = Epf; a.status = e->d_status + e->max_R;
  return a;
}
static EvalArgs eval_args(const drna_engine* e, const char* seqs, int L, int32_t* Ed) {
  EvalArgs a{};
  a.T = e->d_mfeT; a.hp_len = e->d_hp_len; a.bulge_len = e->d_bulge_len; a.int_len = e->d_int_len;
  a.seqs = seqs; a.pt = e->d_pt; a.L = L; a.n_targets = e->n_targets; a.Ed = Ed;
  return a;
}
// two strands of L nucleotides in all, the first one cut long (F4 is allocated by the entry points that fold two strands)
static CoArgs co_args(const drna_engine* e, const char* seqs, int L, int cut, int ld) {
  CoArgs a;
  a.T = e->d_mfeT; a.F = e->d_pfT; a.plan = e->d_plan; a.hp_len = e->d_hp_len; a.hp_w = e->d_hp_w;
  a.scale = e->d_scale; a.eMLb = e->d_eMLb; a.seqs = seqs; a.L = L; a.cut = cut; a.ld = ld;
  a.DuplexInit = e->H.DuplexInit;
  a.eDuplexInit = std::exp(-(double)e->H.DuplexInit * 10.0 / e->H.pf.kT);
  a.wsm = e->d_ws_mfe; a.wsm_stride = (long long)mfe_ws_stride(ld);
  a.wsp = e->d_ws_pf; a.wsp_stride = (long long)pf_ws_stride(ld);
  a.Emfe = e->d_Emfe; a.ss = e->d_ss; a.F4 = e->d_F4; a.status = e->d_status; a.status_pf = e->d_status + e->max_R;
  return a;
}
#ifndef DRNA_PF_HELPER_NMIN
#define DRNA_PF_HELPER_NMIN 95
#endif
constexpr int PF_HELPER_NMIN = DRNA_PF_HELPER_NMIN;       // shorter sequences have too few far split points to repay a second workgroup
                                                          // (tools/pf_helper_lengths.py, R = 64: 90 nt 0.159 against 0.161 ms, 100 nt 0.176 against 0.182, 120 nt 0.215 against 0.228)

// strips of a sequence of length n (0 = not a strip case): widest strip STRIP_WMAX columns; the exchange records of the
// S - 1 strip boundaries must fit tables 0 and 1 of the sequence's workspace
static int strips_for(const drna_engine* e, int n, int ld) {
  if (!e->strips || n > STRIP_NMAX) return 0;
  int S = 0;
  if (n > PF_FAST_NMAX) S = strip_count(n, STRIP_WMAX);
  else if (e->strips == 2 && n > 64) S = 2;
  if (S < 2 || S > STRIP_MAXS) return 0;
  if ((long long)(S - 1) * STRIP_REC > 2ll * ld) return 0;
  return S;
}

// The flags f, ints of them at least, ready for the next epoch: allocated and zeroed on first use or growth.  Flag compares are
// wrap-safe over HALF the 32-bit range only (2^19 epochs of 4096 values): a slot that was never written, or not written for 2^19
// launches (the MFE half of the strips after a long partition-function-only phase, a larger batch than seen before, more strips
// than before), would then read as already published.  Every stream is idle here, so long before that point the flags go back to
// zero and the epoch starts over.
static int flags_ready(drna_engine* e, EpochFlags& f, size_t ints) {
  if (f.ints < ints) {
    if (f.d) (void)hipFree(f.d);
    f.d = nullptr; f.ints = 0;
    HIP_TRY(hipMalloc((void**)&f.d, ints * sizeof(int)));
    f.ints = ints;
  } else if (f.epoch >= f.reset_at) e->flag_resets++;
  else return DRNA_OK;
  HIP_TRY(hipMemset(f.d, 0, f.ints * sizeof(int)));
  f.epoch = 0;
  HIP_TRY(hipDeviceSynchronize());        // the memset runs on the null stream, the kernels on non-blocking streams of their own
  return DRNA_OK;
}
static int flags_next(EpochFlags& f) { return f.epoch = (int)((unsigned)f.epoch + 1u); }   // reset by flags_ready() long before the half range
static int epoch_base(int epoch) { return (int)((unsigned)epoch << 12); }       // of StripLink::base and PfArgs::hbase

// flags (and, for the MFE fold, the record buffer) of the strip kernels, allocated on first use
static int strip_flags(drna_engine* e, bool mfe) {
  const bool first = !e->sflags.d;
  { const int rc = flags_ready(e, e->sflags, (size_t)2 * e->max_R * STRIP_MAXS * 32); if (rc != DRNA_OK) return rc; }
  if (first && getenv("DRNA_STRIP_DEBUG")) {
    HIP_TRY(hipMalloc((void**)&e->d_sclk, (size_t)e->max_R * STRIP_MAXS * 2 * sizeof(long long)));
    HIP_TRY(hipMalloc((void**)&e->d_sdbg, (size_t)2 * e->max_R * 8 * sizeof(int)));
    HIP_TRY(hipMemset(e->d_sdbg, 0, (size_t)2 * e->max_R * 8 * sizeof(int)));
    HIP_TRY(hipDeviceSynchronize());
  }
  if (mfe && !e->d_srec) {
    const int smax = std::min(STRIP_MAXS, strip_count(std::min(e->max_L, STRIP_NMAX), STRIP_WMAX) + 1);
    e->srec_stride = (long long)std::max(smax, 2) * (e->max_L + 2) * MSTRIP_REC;
    HIP_TRY(hipMalloc((void**)&e->d_srec, (size_t)e->srec_stride * e->max_R * sizeof(int32_t)));
  }
  return DRNA_OK;
}

// nseq sequences (slots first_slot ...; idx = their sequence numbers or null) by S strips each
constexpr int SOLO_CALLS = 1000;      // calls with one workgroup per fold after three lost calls in a row (see fallback_streak)
static void launch_pf_strips(drna_engine* e, const PfArgs& a, int nseq, int S, int first_slot, const int* idx, hipStream_t st) {
  StripLink lk;
  lk.flags = e->sflags.d + (size_t)first_slot * STRIP_MAXS * 32;
  lk.base = epoch_base(flags_next(e->sflags));
  lk.nseq = nseq; lk.S = S; lk.idx = idx; lk.pad = strip_pad(S); lk.fault = e->strip_fault;
  lk.dbg = e->d_sdbg ? e->d_sdbg + (size_t)first_slot * 8 : nullptr;
  const int groups = (nseq + 7) / 8;
  hipLaunchKernelGGL(pf_strip_kernel<1024>, dim3(groups * 8 * (S + strip_pad(S))), dim3(1024), 0, st, a, lk);
}

// one pseudoknot round of nseq sequences (slots first_slot ...; idx = their sequence numbers, or null: sequences r0 ...)
static void launch_mfe_strips_round(drna_engine* e, const MfeArgs& a, int nseq, int S, int first_slot, const int* idx, int r0,
                                    hipStream_t st, int round, hipEvent_t after_fill = nullptr) {
  StripRec xr;
  xr.rec = e->d_srec; xr.stride = e->srec_stride;
  const int groups = (nseq + 7) / 8;
  StripLink lk;
  lk.flags = e->sflags.d + ((size_t)e->max_R + first_slot) * STRIP_MAXS * 32;
  lk.base = epoch_base(flags_next(e->sflags));
  lk.nseq = nseq; lk.S = S; lk.idx = idx; lk.r0 = r0; lk.pad = strip_pad(S); lk.fault = e->strip_fault;
  // blocked multiloop splits for the long folds (fold_mfe_strip.hpp, MKT_L).  Alone they win from four strips on (400 nt x 256:
  // 4.86 -> 4.48 ms); beside the partition function's strips only from five on (400 nt: both folds 9.31 -> 9.94 ms, 600 nt x 128:
  // 11.3 -> 9.9 ms) -- unless the MFE fold is a chain of pseudoknot rounds, which then dominates the call (config 5: 10.4 -> 9.6 ms)
  lk.fark = S >= e->mfe_fark_min_strips + ((e->cur_with_pf && a.pk_rounds == 0) ? 1 : 0);
  lk.dbg = e->d_sdbg ? e->d_sdbg + ((size_t)e->max_R + first_slot) * 8 : nullptr;
  lk.clk = e->d_sclk ? e->d_sclk + (size_t)first_slot * STRIP_MAXS * 2 : nullptr;
  if (lk.fark) hipLaunchKernelGGL((mfe_strip_kernel<1024, true>), dim3(groups * 8 * (S + strip_pad(S))), dim3(1024), 0, st, a, lk, xr, round);
  else hipLaunchKernelGGL((mfe_strip_kernel<1024, false>), dim3(groups * 8 * (S + strip_pad(S))), dim3(1024), 0, st, a, lk, xr, round);
  if (after_fill) (void)hipEventRecord(after_fill, st);
  hipLaunchKernelGGL(mfe_strip_trace_kernel, dim3(nseq), dim3(TRACE_WAVES * WAVE), 0, st, a, idx, nseq, round, r0);
}
// MFE fold of nseq sequences by S strips each: per pseudoknot round one launch of the fill and one of the traceback
static void launch_mfe_strips(drna_engine* e, const MfeArgs& a, int nseq, int S, int first_slot, const int* idx, hipStream_t st) {
  if (e->d_sdbg) fprintf(stderr, "mfe strips: rec %p stride %lld max_R %d nseq %d S %d ld %d L %d ws %p\n", (void*)e->d_srec, e->srec_stride, e->max_R, nseq, S, a.ld, a.L, (void*)a.ws);
  for (int round = 0; round <= a.pk_rounds; round++) launch_mfe_strips_round(e, a, nseq, S, first_slot, idx, 0, st, round);
}

static int create_impl(drna_engine* e, const int32_t* params, int n_int32, int device, int max_R, int max_L) {
  if (!params || max_R < 1 || max_L < 1 || max_L > MAXN - 2) {
    e->err = "drna_create: bad argument (1 <= max_L <= 2046, max_R >= 1)";
    return DRNA_ERR_ARG;
  }
  std::string msg = build_tables(params, n_int32, e->H);
  if (!msg.empty()) { e->err = msg; return DRNA_ERR_PARAMS; }
  size_tables(e->H, max_L + 2);
  e->device = device; e->max_R = max_R; e->max_L = max_L;
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  e->cus = prop.multiProcessorCount;
  if (const char* dv = getenv("DRNA_DUAL")) { e->dual = atoi(dv) != 0; e->dual_force = atoi(dv) == 2; }
  if (const char* hv = getenv("DRNA_PF_HELPER")) e->pf_helper = atoi(hv) != 0;
  if (const char* fv = getenv("DRNA_FUSED")) e->fused = atoi(fv) != 0;
  if (const char* mv = getenv("DRNA_MFE_SPLIT")) { const int v = atoi(mv); e->mfe_split = v < 1 ? 1 : v > 8 ? 8 : v; }
  if (const char* fv = getenv("DRNA_MFE_FARK_MIN_STRIPS")) { const int v = atoi(fv); e->mfe_fark_min_strips = v < 1 ? 1 : v; }
  if (const char* sv = getenv("DRNA_STRIPS")) { const int v = atoi(sv); e->strips = v < 0 ? 0 : v > 2 ? 2 : v; }
  HIP_TRY(upload(&e->d_mfeT, &e->H.mfe, 1));
  HIP_TRY(upload(&e->d_pfT, &e->H.pf, 1));
  HIP_TRY(upload(&e->d_plan, &e->H.plan, 1));
  HIP_TRY(upload(&e->d_hp_len, e->H.hp_len.data(), e->H.hp_len.size()));
  HIP_TRY(upload(&e->d_bulge_len, e->H.bulge_len.data(), e->H.bulge_len.size()));
  HIP_TRY(upload(&e->d_int_len, e->H.int_len.data(), e->H.int_len.size()));
  HIP_TRY(upload(&e->d_hp_w, e->H.hp_w.data(), e->H.hp_w.size()));
  HIP_TRY(upload(&e->d_scale, e->H.scale.data(), e->H.scale.size()));
  HIP_TRY(upload(&e->d_eMLb, e->H.eMLb.data(), e->H.eMLb.size()));
  const int ld = max_L + 2;
  {
    // O(ld^2) tables per sequence: 7 fp64 + 5 int32 tables, 12.3 MB at 400 nt.  A batch of 3,200 sequences used to take 39.8 GB;
    // the workspaces now hold at most DRNA_WS_GB (default 8) and a larger batch goes through them in chunks
    double gb = 8.0;
    if (const char* g = getenv("DRNA_WS_GB")) gb = std::max(0.05, atof(g));
    const double per = (double)mfe_ws_stride(ld) * sizeof(int32_t) + (double)pf_ws_stride(ld) * sizeof(double);
    const long long fit = (long long)(gb * 1e9 / per);
    e->ws_slots = (int)std::max(1ll, std::min((long long)max_R, fit));
  }
  size_t bm = mfe_ws_stride(ld) * sizeof(int32_t) * e->ws_slots, bp = pf_ws_stride(ld) * sizeof(double) * e->ws_slots;
  HIP_TRY(hipMalloc((void**)&e->d_ws_mfe, bm));
  HIP_TRY(hipMalloc((void**)&e->d_ws_pf, bp));
  e->ws_bytes = bm + bp;
  HIP_TRY(hipMalloc((void**)&e->d_seqs, (size_t)max_R * max_L));
  HIP_TRY(hipMalloc((void**)&e->d_Epf, (size_t)max_R * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&e->d_Emfe, (size_t)max_R * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&e->d_ss, (size_t)max_R * max_L));
  HIP_TRY(hipHostMalloc((void**)&e->h_status, (size_t)2 * max_R * sizeof(int32_t), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->d_status, e->h_status, 0));
  memset(e->h_status, 0, (size_t)2 * max_R * sizeof(int32_t));
  HIP_TRY(hipHostMalloc((void**)&e->hm_seqs, (size_t)max_R * max_L, hipHostMallocMapped));
  HIP_TRY(hipHostMalloc((void**)&e->hm_ss, (size_t)max_R * max_L, hipHostMallocMapped));
  HIP_TRY(hipHostMalloc((void**)&e->hm_Epf, (size_t)max_R * sizeof(double), hipHostMallocMapped));
  HIP_TRY(hipHostMalloc((void**)&e->hm_Emfe, (size_t)max_R * sizeof(int32_t), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_seqs, e->hm_seqs, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_ss, e->hm_ss, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_Epf, e->hm_Epf, 0));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_Emfe, e->hm_Emfe, 0));
  HIP_TRY(hipStreamCreateWithFlags(&e->s_mfe, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&e->s_pf, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&e->s_eval, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_mfe2, hipEventDisableTiming));
  hipEvent_t* evs[] = {&e->ev_start, &e->ev_end, &e->ev_m0, &e->ev_m1, &e->ev_p0, &e->ev_p1, &e->ev_e0, &e->ev_e1,
                       &e->ev_o0, &e->ev_o1, &e->ev_o2, &e->ev_gate};
  for (hipEvent_t* ev : evs) HIP_TRY(hipEventCreate(ev));
  return DRNA_OK;
}

extern "C" int drna_create(const int32_t* params, int n_int32, int device, int max_R, int max_L, drna_engine** out) {
  if (!out) return DRNA_ERR_ARG;
  *out = nullptr;
  drna_engine* e = new drna_engine();
  int rc = create_impl(e, params, n_int32, device, max_R, max_L);
  if (rc != DRNA_OK) {
    g_create_error = e->err;
    drna_destroy(e);
    return rc;
  }
  *out = e;
  return DRNA_OK;
}

extern "C" void drna_destroy(drna_engine* e) {
  if (!e) return;
  void* bufs[] = {e->d_mfeT, e->d_pfT, e->d_plan, e->d_hp_len, e->d_bulge_len, e->d_int_len, e->d_hp_w, e->d_scale,
                  e->d_eMLb, e->d_ws_mfe, e->d_ws_pf, e->d_seqs, e->d_Epf, e->d_Emfe, e->d_ss, e->d_Ed, e->d_pt,
                  e->d_ws_out, e->d_edef, e->d_rg, e->d_rpt, e->d_rpt_off, e->d_F4, e->d_ws_kb, e->d_kbE, e->d_kbss,
                  e->dflags.d, e->d_xs, e->d_xa_mfe, e->d_xb_mfe, e->sflags.d, e->d_srec, e->d_sdbg, e->d_sclk, e->pflags.d, e->d_q5s, e->d_cocols, e->d_mea_pt, e->d_nopair};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (e->h_status) (void)hipHostFree(e->h_status);
  void* hm[] = {e->hm_seqs, e->hm_ss, e->hm_Epf, e->hm_Emfe, e->hm_Ed, e->hm_F4, e->h_clk};
  for (void* b : hm)
    if (b) (void)hipHostFree(b);
  hipStream_t ss[] = {e->s_mfe, e->s_pf, e->s_eval};
  if (e->ev_mfe2) (void)hipEventDestroy(e->ev_mfe2);
  for (hipStream_t s : ss)
    if (s) (void)hipStreamDestroy(s);
  hipEvent_t evs[] = {e->ev_start, e->ev_end, e->ev_m0, e->ev_m1, e->ev_p0, e->ev_p1, e->ev_e0, e->ev_e1,
                      e->ev_o0, e->ev_o1, e->ev_o2, e->ev_gate};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  delete e;
}

extern "C" int drna_abi_version(void) { return DRNA_ABI_VERSION; }

static int poison_scratch(drna_engine* e, int byte);      // option "poison", at the end of the file

extern "C" int drna_set_option(drna_engine* e, const char* name, int value) {
  if (!e || !name) return DRNA_ERR_ARG;
  if (!strcmp(name, "dual") || !strcmp(name, "strips") || !strcmp(name, "pf_helper") || !strcmp(name, "fused")) { e->fallback_streak = 0; e->solo_left = 0; }
  if (!strcmp(name, "fused")) { e->fused = value != 0; return DRNA_OK; }
  if (!strcmp(name, "dual")) { e->dual = value != 0; e->dual_force = value == 2; return DRNA_OK; }
  if (!strcmp(name, "strips")) { e->strips = value < 0 ? 0 : value > 2 ? 2 : value; return DRNA_OK; }
  if (!strcmp(name, "pf_helper")) { e->pf_helper = value != 0; return DRNA_OK; }
  if (!strcmp(name, "cofold_lds")) { e->cofold_lds = value != 0; return DRNA_OK; }
  if (!strcmp(name, "subopt_lds")) { e->subopt_lds = value != 0; return DRNA_OK; }
  if (!strcmp(name, "edef_lds")) { e->edef_lds = value != 0; return DRNA_OK; }
  if (!strcmp(name, "access_lds")) { e->access_lds = value != 0; e->access_lds_force = value == 2; return DRNA_OK; }
  if (!strcmp(name, "mea_lds")) { e->mea_lds = value != 0; return DRNA_OK; }
  if (!strcmp(name, "self_dimer_lds")) { e->self_dimer_lds = value != 0; return DRNA_OK; }
  if (!strcmp(name, "helper_fault")) { e->helper_fault = value != 0; return DRNA_OK; }
  if (!strcmp(name, "strip_fault")) { e->strip_fault = value != 0; return DRNA_OK; }
  if (!strcmp(name, "mfe_fark_min_strips")) { e->mfe_fark_min_strips = value < 1 ? 1 : value; return DRNA_OK; }
  if (!strcmp(name, "mfe_split")) { e->mfe_split = value < 1 ? 1 : value > 8 ? 8 : value; return DRNA_OK; }
  if (!strcmp(name, "debug_epoch")) { e->sflags.epoch = e->dflags.epoch = e->pflags.epoch = value; return DRNA_OK; }     // tests: jump near the reset point
  if (!strcmp(name, "poison")) {                                                                                         // tests: a stale read shows in the values
    if (value < 0 || value > 255) { e->err = "drna_set_option: poison takes a byte, 0 .. 255"; return DRNA_ERR_ARG; }
    return poison_scratch(e, value);
  }
  e->err = std::string("drna_set_option: unknown option ") + name;
  return DRNA_ERR_ARG;
}

// diagnostics (DRNA_STRIP_DEBUG=1): start / end wall clocks (100 MHz ticks) of the MFE strip workgroups of the last launch,
// out[slot][strip][2]; returns the number of slots copied (0 without the debug buffers)
extern "C" int drna_debug_strip_clocks(drna_engine* e, long long* out, int nslots) {
  if (!e || !e->d_sclk || !out) return 0;
  const int m = std::min(nslots, e->max_R);
  if (hipMemcpy(out, e->d_sclk, (size_t)m * STRIP_MAXS * 2 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return m;
}

extern "C" int drna_get_option(const drna_engine* e, const char* name, int* value) {
  if (!e || !name || !value) return DRNA_ERR_ARG;
  if (!strcmp(name, "dual")) { *value = e->dual ? (e->dual_force ? 2 : 1) : 0; return DRNA_OK; }
  if (!strcmp(name, "strips")) { *value = e->strips; return DRNA_OK; }
  if (!strcmp(name, "pf_helper")) { *value = e->pf_helper ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "fused")) { *value = e->fused ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "cofold_lds")) { *value = e->cofold_lds ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "cofold_lds_max")) { *value = CO_LDS_MAX; return DRNA_OK; }
  if (!strcmp(name, "edef_lds")) { *value = e->edef_lds ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "edef_lds_max")) { *value = EDEF_LDS_HOST_MAX; return DRNA_OK; }     // what the host sends there; the kernel holds EDEF_LDS_MAX
  if (!strcmp(name, "cofold_edef_lds_max")) { *value = CO_EDEF_LDS_MAX; return DRNA_OK; }
  if (!strcmp(name, "edef_lds_calls")) { *value = e->edef_lds_calls; return DRNA_OK; }
  if (!strcmp(name, "access_lds")) { *value = e->access_lds ? (e->access_lds_force ? 2 : 1) : 0; return DRNA_OK; }
  if (!strcmp(name, "access_lds_max")) { *value = ACCESS_LDS_HOST_MAX; return DRNA_OK; }     // what the host sends there ...
  if (!strcmp(name, "access_lds_kernel_max")) { *value = ACCESS_LDS_MAX; return DRNA_OK; }   // ... and what the kernel holds
  if (!strcmp(name, "access_lds_calls")) { *value = e->access_lds_calls; return DRNA_OK; }
  if (!strcmp(name, "sample_calls")) { *value = e->sample_calls; return DRNA_OK; }
  if (!strcmp(name, "cofold_sample_calls")) { *value = e->cofold_sample_calls; return DRNA_OK; }
  if (!strcmp(name, "mea_lds")) { *value = e->mea_lds ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "mea_lds_max")) { *value = MEA_LDS_MAX; return DRNA_OK; }
  if (!strcmp(name, "mea_calls")) { *value = e->mea_calls; return DRNA_OK; }
  if (!strcmp(name, "mea_candidates")) { *value = e->mea_cands; return DRNA_OK; }
  if (!strcmp(name, "subopt_lds")) { *value = e->subopt_lds ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "subopt_lds_max")) { *value = SUB_LDS_MAX; return DRNA_OK; }
  if (!strcmp(name, "self_dimer_lds")) { *value = e->self_dimer_lds ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "self_dimer_lds_max")) { *value = SD_LDS_MAX; return DRNA_OK; }
  if (!strcmp(name, "last_fused")) { *value = e->last_fused ? 1 : 0; return DRNA_OK; }
  if (!strcmp(name, "fused_blocks_per_cu")) { *value = e->fused_blocks_per_cu; return DRNA_OK; }
  if (!strcmp(name, "pair_blocks_per_cu")) { *value = e->pair_blocks_per_cu; return DRNA_OK; }
  if (!strcmp(name, "sync_fallbacks")) { *value = e->sync_fallbacks; return DRNA_OK; }
  if (!strcmp(name, "solo_calls_left")) { *value = e->solo_left; return DRNA_OK; }
  if (!strcmp(name, "last_workgroups")) { *value = e->last_wgs; return DRNA_OK; }
  if (!strcmp(name, "mc_threads_used")) { *value = 1; return DRNA_OK; }       // drna_mc_run's host work runs on the calling thread
  if (!strcmp(name, "workspace_slots")) { *value = e->ws_slots; return DRNA_OK; }
  if (!strcmp(name, "flag_resets")) { *value = e->flag_resets; return DRNA_OK; }
  if (!strcmp(name, "motifs")) { *value = (int)e->motifs.motifs.size(); return DRNA_OK; }      // set by drna_set_motifs only
  if (!strcmp(name, "debug_epoch")) { *value = std::max(e->pflags.epoch, std::max(e->sflags.epoch, e->dflags.epoch)); return DRNA_OK; }
  return DRNA_ERR_ARG;
}

extern "C" const char* drna_last_error(const drna_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

// pair table p[1..L] (partner or 0, p zeroed by the caller) of the target structure s[0..L): only '(' and ')' pair, every other
// character is unpaired
static int target_pairs(drna_engine* e, const char* who, const char* s, int L, short* p) {
  std::vector<int> stk;
  for (int i = 1; i <= L; i++) {
    if (s[i - 1] == '(') stk.push_back(i);
    else if (s[i - 1] == ')') {
      if (stk.empty()) { e->err = std::string(who) + ": unbalanced ')'"; return DRNA_ERR_STRUCTURE; }
      const int o = stk.back(); stk.pop_back();
      p[o] = (short)i; p[i] = (short)o;
    }
  }
  if (!stk.empty()) { e->err = std::string(who) + ": unbalanced '('"; return DRNA_ERR_STRUCTURE; }
  return DRNA_OK;
}

extern "C" int drna_set_targets(drna_engine* e, int n_targets, int L, const char* targets) {
  if (!e) return DRNA_ERR_ARG;
  if (n_targets < 0 || L < 1 || L > e->max_L || (n_targets > 0 && !targets)) {
    e->err = "drna_set_targets: bad argument";
    return DRNA_ERR_ARG;
  }
  std::vector<short> pt((size_t)n_targets * (L + 2), 0);
  for (int k = 0; k < n_targets; k++) {
    const int rc = target_pairs(e, "drna_set_targets", targets + (size_t)k * L, L, pt.data() + (size_t)k * (L + 2));
    if (rc != DRNA_OK) return rc;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (e->d_pt) { (void)hipFree(e->d_pt); e->d_pt = nullptr; }
  if (e->d_Ed) { (void)hipFree(e->d_Ed); e->d_Ed = nullptr; }
  e->n_targets = n_targets; e->L_targets = L;
  if (n_targets) {
    HIP_TRY(upload(&e->d_pt, pt.data(), pt.size()));
    HIP_TRY(hipMalloc((void**)&e->d_Ed, (size_t)e->max_R * n_targets * sizeof(int32_t)));
  }
  return DRNA_OK;
}

// Folds by several workgroups that wait for each other (fold_mfe_dual.hpp, pf_kfar_helper) need ALL their workgroups resident at
// once.  Every such launch is therefore sized against the occupancy query, which is the check hipLaunchCooperativeKernel makes
// (that call itself costs ~17 us more per launch, MI355X_MICROARCH.md 'coop-launch', and gives the same residency as a plain
// launch): workgroups of all concurrent launches <= blocks per CU x CUs.  What remains outside the engine's control is another
// process on the same GPU; the bounded waits and the one-workgroup fallback cover that (ST_SYNC).
static int pair_blocks_per_cu(drna_engine* e) {
  if (e->pair_blocks_per_cu < 0) {
    int a = 0, b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, mfe_dual_kernel<1024>, 1024, 0) != hipSuccess) a = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, pf_lds_kernel<1024, false>, 1024, 0) != hipSuccess) b = 0;      // (the instance of the helper launches)
    e->pair_blocks_per_cu = std::min(a, b);
  }
  return e->pair_blocks_per_cu;
}

// The fused launch's workgroups wait for each other, so the whole grid must be resident at once: the grid is checked against
// the occupancy query (what hipLaunchCooperativeKernel would check, without its ~17 us per launch)
static bool fused_grid_fits(drna_engine* e, int R) {
  if (e->fused_blocks_per_cu < 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, score_fused_kernel<1024>, 1024, 0) != hipSuccess) nb = 0;
    e->fused_blocks_per_cu = nb;
  }
  return (long long)fused_grid(R) <= (long long)e->fused_blocks_per_cu * e->cus;
}

// The status words of the R sequences just folded (MFE fold before partition function) as a return code, with the message in
// e->err; the first sequence that failed decides.  Position q is the caller's sequence order[q] (ragged batches) or r_base + q.
// A lost partner of a multi-workgroup fold (ST_SYNC) is DRNA_ERR_INTERNAL and sets *lost: the caller may redo the call by fold_solo
static int fold_status(drna_engine* e, int R, bool want_mfe, bool want_pf, const int* order, int r_base, const char* internal_msg,
                       bool* lost = nullptr) {
  for (int q = 0; q < R; q++) {
    const int sm = want_mfe ? e->h_status[q] : ST_OK, sp = want_pf ? e->h_status[e->max_R + q] : ST_OK;
    const int st = sm != ST_OK ? sm : sp;
    if (st == ST_OK) continue;
    const int r = order ? order[q] : r_base + q;
    char buf[192];
    if (st == ST_BAD_CHAR) snprintf(buf, sizeof buf, "sequence %d holds a character other than A C G U T", r);
    else if (st == ST_PF_RANGE) snprintf(buf, sizeof buf, "sequence %d: partition function left the fp64 range (pf_scale too small/large)", r);
    else if (st == ST_SYNC) snprintf(buf, sizeof buf, "sequence %d: the workgroups of the fold lost each other (a wait expired)", r);
    else snprintf(buf, sizeof buf, "sequence %d: %s", r, internal_msg);
    e->err = buf;
    if (lost) *lost = st == ST_SYNC;
    return st == ST_BAD_CHAR ? DRNA_ERR_SEQUENCE : st == ST_PF_RANGE ? DRNA_ERR_PF_RANGE : DRNA_ERR_INTERNAL;
  }
  return DRNA_OK;
}

// fold() with one workgroup per fold: the strip kernels, the two-workgroup MFE kernel and the partition function's helpers off, so
// only the general and LDS-resident kernels run, which wait for nobody
template <class F>
static int fold_solo(drna_engine* e, F&& fold) {
  const int s_strips = e->strips;
  const bool s_dual = e->dual, s_help = e->pf_helper;
  e->in_fallback = true; e->strips = 0; e->dual = false; e->pf_helper = false;
  const int rc = fold();
  e->strips = s_strips; e->dual = s_dual; e->pf_helper = s_help; e->in_fallback = false;
  return rc;
}
// HIP promises no dispatch order: a multi-workgroup fold whose bounded wait expired is not an error of the batch -- the whole
// call is redone by fold_solo
template <class F>
static int redo_solo(drna_engine* e, F&& fold) {
  const int rc = fold_solo(e, fold);
  e->sync_fallbacks++;
  if (++e->fallback_streak >= 3) { e->fallback_streak = 0; e->solo_left = SOLO_CALLS; }
  return rc;
}

static void reset_status(drna_engine* e) {
  for (int k = 0; k < 2 * e->max_R; k++) e->h_status[k] = ST_OK;
}

// Which kernels a uniform batch takes and how many workgroups each fold puts on the chip.  Decided once per call (a redone call
// plans again, with the multi-workgroup paths off); the prepare, enqueue and drain steps and last_workgroups all read it.
struct FoldPlan {
  bool want_pf, want_mfe, want_pk, want_ev;
  bool dual;                      // MFE fold by a main and a helper workgroup per sequence (fold_mfe_dual.hpp)
  bool pf_help, ev_in_pf;         // partition function with a helper workgroup per sequence (pf_kfar_helper), which also evaluates E(targets)
  bool fused;                     // both folds in ONE launch, 4 R workgroups resident side by side (fold_fused.hpp)
  int pf_strips, mfe_strips;      // strips of columns per sequence, one workgroup each (fold_pf_strip.hpp); 0: not by strips
  int mfe_wgs, pf_wgs;            // workgroups of each fold
};
static FoldPlan plan_uniform(drna_engine* e, int R, int L, uint32_t flags) {
  FoldPlan p{};
  p.want_pf = flags & DRNA_NEED_PF; p.want_mfe = flags & (DRNA_NEED_MFE | DRNA_NEED_PK);
  p.want_pk = flags & DRNA_NEED_PK; p.want_ev = flags & DRNA_NEED_EVAL;
  // small batches leave most CUs idle with one workgroup per fold (R = 64: 128 workgroups on 256 CUs): the MFE fold then
  // takes a main and a helper workgroup per sequence (fold_mfe_dual.hpp; the same split of the partition function did not
  // pay).  Needs 4 R <= CUs; larger batches keep the one-workgroup kernels, which saturate the chip by themselves
  // (R = 64 x L = 200: the MFE fold takes 0.50 instead of 0.59 ms, 1.65 instead of 1.81 ms with the pseudoknot re-folds; the
  // partition function running beside it loses 1 % to the busier chip's lower clock)
  // Shorter sequences do not repay the hand-shake: break-even (tools/dual_lengths.py, R = 64, with a sequence's two workgroups on
  // one XCD) at n = 120 without pseudoknot rounds (n = 130: 0.275 against 0.292 ms, n = 160: 0.336 against 0.383) and at n = 165
  // with them (their re-folds of masked sequences have little for the helper to do).
  const long long resident = (long long)e->cus * (e->dual || e->pf_helper ? pair_blocks_per_cu(e) : 1);   // workgroups the chip holds at once
  p.dual = e->dual && L <= MFE_FAST_NMAX && L > 2 * TURN + 2 && 4ll * R <= resident &&
           (L >= (p.want_pk ? 170 : 125) || e->dual_force);
  // longer sequences (and, as an option, short ones in small batches): the folds by strips of columns
  p.pf_strips = p.want_pf ? strips_for(e, L, L + 2) : 0;
  p.mfe_strips = p.want_mfe ? strips_for(e, L, L + 2) : 0;
  p.mfe_wgs = p.want_mfe ? (p.dual ? 2 * R : p.mfe_strips ? R * p.mfe_strips : R) : 0;
  // partition function of a small batch: a helper workgroup per sequence on a CU that would idle takes the far multiloop split
  // points (the main workgroup's vector-memory path is what they saturate); needs room for 2 R workgroups beside the MFE fold's
  p.pf_help = p.want_pf && e->pf_helper && !p.pf_strips && L <= PF_FAST_NMAX && L >= PF_HELPER_NMIN &&
              2ll * R + p.mfe_wgs <= resident;
  p.pf_wgs = p.want_pf ? (p.pf_strips ? R * p.pf_strips : p.pf_help ? 2 * R : R) : 0;
  p.ev_in_pf = p.want_ev && p.pf_help;
  p.fused = e->fused && p.dual && p.pf_help && p.want_mfe && p.want_pf && (!p.want_ev || p.ev_in_pf) && fused_grid_fits(e, R);
  return p;
}

// what the planned kernels need before the first launch: their hand-over flags at a fresh epoch, the exchange rows of the
// two-workgroup MFE fold (362 KB per sequence, so they grow with the batches seen and not to max_R) and the fused launch's clocks
static int prepare_folds(drna_engine* e, const FoldPlan& p, int R) {
  if (p.dual) {
    { const int rc = flags_ready(e, e->dflags, (size_t)2 * R * 64); if (rc != DRNA_OK) return rc; }
    if (e->dual_cap < R) {
      for (int32_t** b : {&e->d_xs, &e->d_xa_mfe, &e->d_xb_mfe}) { if (*b) (void)hipFree(*b); *b = nullptr; }
      e->dual_cap = 0;
      const size_t rows = (size_t)2 * (MFE_FAST_NMAX + 2) * XP;
      HIP_TRY(hipMalloc((void**)&e->d_xs, (size_t)R * 256 * sizeof(int32_t)));
      HIP_TRY(hipMalloc((void**)&e->d_xa_mfe, (size_t)R * rows * sizeof(int32_t)));
      HIP_TRY(hipMalloc((void**)&e->d_xb_mfe, (size_t)R * rows * sizeof(int32_t)));
      e->dual_cap = R;
    }
    flags_next(e->dflags);
  }
  if (p.pf_help) {
    { const int rc = flags_ready(e, e->pflags, (size_t)R * 64); if (rc != DRNA_OK) return rc; }
    flags_next(e->pflags);
  }
  if (p.pf_strips || p.mfe_strips) { const int rc = strip_flags(e, p.mfe_strips != 0); if (rc != DRNA_OK) return rc; }
  if (p.fused && e->clk_cap < fused_grid(R)) {
    if (e->h_clk) (void)hipHostFree(e->h_clk);
    e->h_clk = nullptr; e->clk_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&e->h_clk, (size_t)2 * fused_grid(R) * sizeof(long long), hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void**)&e->d_clk, e->h_clk, 0));
    e->clk_cap = fused_grid(R);
  }
  return DRNA_OK;
}

// one uniform batch on its way through the streams: plan, kernel arguments, and what the enqueue step leaves for the drain step
struct FoldCall {
  int R, L;
  FoldPlan p;
  MfeArgs ma; PfArgs pa; EvalArgs ev; DualLink lk;
  bool mfe_first;                 // the MFE fold is enqueued before the partition function
  hipStream_t s_ev;               // stream of the evaluation kernel
  bool pf_gated;                  // the partition function's launch waits for ev_gate (enqueue_mfe decides, enqueue_pf obeys)
};

static int enqueue_pf(drna_engine* e, const FoldCall& c) {
  const FoldPlan& p = c.p; const int R = c.R;
  if (c.pf_gated) HIP_TRY(hipStreamWaitEvent(e->s_pf, e->ev_gate, 0));
  HIP_TRY(hipEventRecord(e->ev_p0, e->s_pf));
  if (p.pf_strips) launch_pf_strips(e, c.pa, R, p.pf_strips, 0, nullptr, e->s_pf);
  else if (p.pf_help)
    hipLaunchKernelGGL((pf_lds_kernel<1024, false>), dim3(pair_grid(R)), dim3(1024), 0, e->s_pf, c.pa, p.ev_in_pf ? c.ev : EvalArgs{}, R);
  else if (c.L <= PF_FAST_NMAX)
    hipLaunchKernelGGL(pf_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, c.pa, EvalArgs{}, R);
  else hipLaunchKernelGGL(pf_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, c.pa);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_p1, e->s_pf));
  return DRNA_OK;
}
static int enqueue_mfe(drna_engine* e, FoldCall& c) {
  const FoldPlan& p = c.p; const MfeArgs& ma = c.ma; const int R = c.R;
  // An MFE fold with pseudoknot rounds on the strip path is a chain of launches whose later links are sparse (only sequences that
  // found a pair fold again), the partition function is one dense launch.  On a chip the first fill already fills (R x strips >=
  // CUs) the partition function is therefore started when the last-but-one round has been queued: it runs beside the sparse rounds
  // instead of halving the CUs of the dense first ones (400 nt x 128: 10.6 -> 9.0 ms, x 256: 19.3 -> 16.5 ms; on a chip with idle CUs
  // it would only delay the partition function: 400 nt x 32 5.4 -> 5.7 ms).  DRNA_PF_GATE=-1 switches it off, k >= 0 forces round k.
  static const int pf_gate_env = getenv("DRNA_PF_GATE") ? atoi(getenv("DRNA_PF_GATE")) : -2;
  static const int pf_gate_part = getenv("DRNA_PF_GATE_PART") ? atoi(getenv("DRNA_PF_GATE_PART")) : 0;
  HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
  if (p.dual) hipLaunchKernelGGL(mfe_dual_kernel<1024>, dim3(pair_grid(R)), dim3(1024), 0, e->s_mfe, ma, c.lk, R);
  else if (p.mfe_strips && ma.pk_rounds > 0 && R >= 16 * e->mfe_split && e->mfe_split > 1) {
    // every round is a fill launch and a traceback launch (one wave per sequence, ~0.2 ms with the chip idle): the batch goes
    // in parts on two streams, so that one part's traceback runs under another part's fill
    const int np = e->mfe_split, per = ((R + np - 1) / np + 7) / 8 * 8;
    const int pf_gate_round = pf_gate_env >= -1 ? pf_gate_env : (p.pf_strips && p.mfe_wgs >= e->cus && ma.pk_rounds >= 2) ? ma.pk_rounds - 1 : -1;
    for (int round = 0; round <= ma.pk_rounds; round++) {
      for (int part = 0, r0 = 0; r0 < R; part++, r0 += per) {
        const bool gate_here = round == pf_gate_round && p.want_pf && part == pf_gate_part;
        launch_mfe_strips_round(e, ma, std::min(per, R - r0), p.mfe_strips, r0, nullptr, r0, (part & 1) ? e->s_eval : e->s_mfe, round,
                                gate_here ? e->ev_gate : nullptr);
        if (gate_here) c.pf_gated = true;
      }
    }
    HIP_TRY(hipEventRecord(e->ev_mfe2, e->s_eval));
    HIP_TRY(hipStreamWaitEvent(e->s_mfe, e->ev_mfe2, 0));
  } else if (p.mfe_strips) launch_mfe_strips(e, ma, R, p.mfe_strips, 0, nullptr, e->s_mfe);
  else if (c.L <= MFE_FAST_NMAX) hipLaunchKernelGGL(mfe_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, ma);
  else hipLaunchKernelGGL(mfe_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, ma);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
  return DRNA_OK;
}
static int enqueue_eval(drna_engine* e, const FoldCall& c) {
  if (c.p.ev_in_pf) return DRNA_OK;
  HIP_TRY(hipEventRecord(e->ev_e0, c.s_ev));
  hipLaunchKernelGGL(eval_kernel, dim3(c.R * e->n_targets), dim3(WAVE), 0, c.s_ev, c.ev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_e1, c.s_ev));
  return DRNA_OK;
}
// Every stream of the engine is idle here (each call drains them before it returns), so nothing has to be fenced at the start.
// Small batches (the headline shape) take both folds in ONE launch; otherwise the two folds run side by side on disjoint CUs
// and a launch costs ~10 us, so the one that took longer in the previous call is enqueued first
static int enqueue_folds(drna_engine* e, FoldCall& c) {
  const FoldPlan& p = c.p;
  e->last_fused = p.fused;
  e->last_wgs = p.mfe_wgs + p.pf_wgs;
  if (p.fused) {
    // (no event pair around the launch: every reported time of this path comes from the blocks' own clock stamps, drain_folds)
    hipLaunchKernelGGL(score_fused_kernel<1024>, dim3(fused_grid(c.R)), dim3(1024), 0, e->s_mfe, c.ma, c.lk, c.pa, c.ev, c.R, e->d_clk);
    HIP_TRY(hipGetLastError());
    return DRNA_OK;
  }
  c.mfe_first = p.want_mfe && (!p.want_pf || e->timing[0] > e->timing[1]);
  // the evaluation kernel (~20 us) rides in FRONT of the shorter fold on that fold's stream: one stream less to drain at the end
  c.s_ev = !(p.want_mfe && p.want_pf) ? e->s_eval : c.mfe_first ? e->s_pf : e->s_mfe;
  if (c.mfe_first) { const int rc = enqueue_mfe(e, c); if (rc != DRNA_OK) return rc; }
  if (p.want_ev && c.s_ev == e->s_pf) { const int rc = enqueue_eval(e, c); if (rc != DRNA_OK) return rc; }
  if (p.want_pf) { const int rc = enqueue_pf(e, c); if (rc != DRNA_OK) return rc; }
  if (p.want_ev && c.s_ev == e->s_mfe) { const int rc = enqueue_eval(e, c); if (rc != DRNA_OK) return rc; }
  if (p.want_mfe && !c.mfe_first) { const int rc = enqueue_mfe(e, c); if (rc != DRNA_OK) return rc; }
  if (p.want_ev && c.s_ev == e->s_eval) { const int rc = enqueue_eval(e, c); if (rc != DRNA_OK) return rc; }
  return DRNA_OK;
}

// wait for the kernels of the call and fill e->timing (MFE, partition function, evaluation, total; ms)
static int drain_folds(drna_engine* e, const FoldCall& c) {
  const FoldPlan& p = c.p;
  if (p.fused) {
    HIP_TRY(hipStreamSynchronize(e->s_mfe));
    // per-fold times from the blocks' own clocks (100 MHz): first start of any block to the last end of the fold's blocks;
    // the total is the later of the two ends
    const int grid = fused_grid(c.R);
    long long t0 = 0, end_mfe = 0, end_pf = 0;
    bool first = true;
    for (int b = 0; b < grid; b++) {
      int r, role;
      fused_block_role(b, r, role, grid);
      if (r >= c.R) continue;
      const long long s0 = e->h_clk[2 * b], s1 = e->h_clk[2 * b + 1];
      if (first || s0 < t0) t0 = s0;
      first = false;
      if (role <= ROLE_MFE_HELPER) { if (s1 > end_mfe) end_mfe = s1; } else if (s1 > end_pf) end_pf = s1;
    }
    e->timing[0] = (float)((end_mfe - t0) * 1e-5); e->timing[1] = (float)((end_pf - t0) * 1e-5);
    e->timing[2] = 0.f; e->timing[3] = std::max(e->timing[0], e->timing[1]);
    return DRNA_OK;
  }
  // join on the host: the streams are drained one after the other (a device-side join -- stream-wait-event packets
  // plus an end marker -- costs ~15 us after the last kernel); "total" = first start event to the latest end event
  const bool ev_own = p.want_ev && !p.ev_in_pf;          // the evaluation ran as a kernel of its own
  if (ev_own && c.s_ev == e->s_eval) HIP_TRY(hipStreamSynchronize(e->s_eval));
  if (c.mfe_first && p.want_pf) HIP_TRY(hipStreamSynchronize(e->s_pf));
  if (p.want_mfe) HIP_TRY(hipStreamSynchronize(e->s_mfe));
  if (!c.mfe_first && p.want_pf) HIP_TRY(hipStreamSynchronize(e->s_pf));
  e->timing[0] = e->timing[1] = e->timing[2] = e->timing[3] = 0.f;
  if (p.want_mfe) HIP_TRY(hipEventElapsedTime(&e->timing[0], e->ev_m0, e->ev_m1));
  if (p.want_pf) HIP_TRY(hipEventElapsedTime(&e->timing[1], e->ev_p0, e->ev_p1));
  if (ev_own) HIP_TRY(hipEventElapsedTime(&e->timing[2], e->ev_e0, e->ev_e1));
  hipEvent_t first = c.mfe_first ? e->ev_m0 : p.want_pf ? e->ev_p0 : e->ev_e0;
  float t = 0.f;
  if (p.want_mfe) { HIP_TRY(hipEventElapsedTime(&t, first, e->ev_m1)); e->timing[3] = std::max(e->timing[3], t); }
  if (p.want_pf) { HIP_TRY(hipEventElapsedTime(&t, first, e->ev_p1)); e->timing[3] = std::max(e->timing[3], t); }
  if (ev_own) { HIP_TRY(hipEventElapsedTime(&t, first, e->ev_e1)); e->timing[3] = std::max(e->timing[3], t); }
  return DRNA_OK;
}

// one batch that fits the workspaces; its sequences are the caller's r_base, r_base + 1, ...
static int score_batch_impl(drna_engine* e, int R, int L, const char* d_seqs, uint32_t flags, double* d_Epf, int32_t* d_Emfe,
                            char* d_mfe_ss, int32_t* d_Ed, int r_base) {
  HIP_TRY(hipSetDevice(e->device));
  // 1. plan (here, inside the call: fold_solo has switched the multi-workgroup paths off before a redone call gets here)
  FoldCall c{R, L, plan_uniform(e, R, L, flags)};
  const FoldPlan& p = c.p;
  // 2. prepare
  { const int rc = prepare_folds(e, p, R); if (rc != DRNA_OK) return rc; }
  reset_status(e);
  e->cur_with_pf = p.want_pf;
  c.ev = p.want_ev ? eval_args(e, d_seqs, L, d_Ed) : EvalArgs{};
  c.ma = mfe_args(e, d_seqs, L, L + 2, p.want_pk ? 3 : 0, d_Emfe, d_mfe_ss);
  c.pa = pf_args(e, d_seqs, L, L + 2, d_Epf);
  if (p.pf_help) { c.pa.helper = e->helper_fault ? 2 : 1; c.pa.hflags = e->pflags.d; c.pa.hbase = epoch_base(e->pflags.epoch); }
  c.lk.flagA = e->dflags.d; c.lk.flagB = e->dflags.d;
  c.lk.xs = e->d_xs; c.lk.xa = e->d_xa_mfe; c.lk.xb = e->d_xb_mfe; c.lk.epoch = e->dflags.epoch;
  // 3. enqueue, 4. drain and time
  { const int rc = enqueue_folds(e, c); if (rc != DRNA_OK) return rc; }
  { const int rc = drain_folds(e, c); if (rc != DRNA_OK) return rc; }
  // 5. status; a lost attempt (up to the wait budget) is not a kernel time and stays out of the sums
  bool lost = false;
  const int rc = fold_status(e, R, p.want_mfe, p.want_pf, nullptr, r_base, "traceback could not reproduce a table value", &lost);
  if (lost && !e->in_fallback)
    return redo_solo(e, [&] { return score_batch_impl(e, R, L, d_seqs, flags, d_Epf, d_Emfe, d_mfe_ss, d_Ed, r_base); });
  for (int k = 0; k < 4; k++) e->timing_sum[k] += e->timing[k];
  e->timing_sum[4] += 1.0;
  if (lost && e->d_sdbg) {
    std::vector<int> dbg((size_t)2 * e->max_R * 8);
    (void)hipMemcpy(dbg.data(), e->d_sdbg, dbg.size() * sizeof(int), hipMemcpyDeviceToHost);
    for (size_t k = 0; k < dbg.size(); k += 8)
      if (dbg[k]) fprintf(stderr, "strip debug slot %zu: strip %d step %d saw flag %d (base %d: %d) block %d n %d\n", k / 8, dbg[k] - 1, dbg[k + 1],
                          dbg[k + 2], dbg[k + 3], dbg[k + 2] - dbg[k + 3], dbg[k + 4], dbg[k + 5]);
  }
  if (rc == DRNA_OK && !e->in_fallback) e->fallback_streak = 0;          // nobody lost anybody
  return rc;
}

// argument check of the two uniform entry points (host and device buffers)
static int score_check(drna_engine* e, int R, int L, const char* seqs, uint32_t flags, const double* Epf, const int32_t* Emfe,
                       const char* mfe_ss, const int32_t* Ed) {
  const bool want_pf = flags & DRNA_NEED_PF, want_mfe = flags & (DRNA_NEED_MFE | DRNA_NEED_PK), want_ev = flags & DRNA_NEED_EVAL;
  if (R >= 1 && R <= e->max_R && L >= 1 && L <= e->max_L && seqs && (!want_pf || Epf) && (!want_mfe || (Emfe && mfe_ss)) &&
      (!want_ev || Ed)) return DRNA_OK;
  e->err = "drna_score_batch: bad argument (R, L within the engine's limits; output pointers for every requested flag)";
  return DRNA_ERR_ARG;
}

extern "C" int drna_score_batch_device(drna_engine* e, int R, int L, const char* d_seqs, uint32_t flags, double* d_Epf,
                                       int32_t* d_Emfe, char* d_mfe_ss, int32_t* d_Ed) {
  if (!e) return DRNA_ERR_ARG;
  { const int rc = score_check(e, R, L, d_seqs, flags, d_Epf, d_Emfe, d_mfe_ss, d_Ed); if (rc != DRNA_OK) return rc; }
  if ((flags & DRNA_NEED_EVAL) && (e->n_targets < 1 || e->L_targets != L)) {
    e->err = "drna_score_batch: DRNA_NEED_EVAL needs drna_set_targets() with the same L";
    return DRNA_ERR_ARG;
  }
  // more sequences than the workspaces hold (DRNA_WS_GB): one sub-batch of ws_slots after the other; last_timing = their sums
  auto sub_batches = [&]() -> int {
    const int nt = std::max(1, e->n_targets);
    float sum[4] = {0, 0, 0, 0};
    for (int r0 = 0; r0 < R; r0 += e->ws_slots) {
      const int m = std::min(e->ws_slots, R - r0);
      const int rc = score_batch_impl(e, m, L, d_seqs + (size_t)r0 * L, flags, d_Epf ? d_Epf + r0 : nullptr, d_Emfe ? d_Emfe + r0 : nullptr,
                                      d_mfe_ss ? d_mfe_ss + (size_t)r0 * L : nullptr, d_Ed ? d_Ed + (size_t)r0 * nt : nullptr, r0);
      if (rc != DRNA_OK) return rc;
      for (int k = 0; k < 4; k++) sum[k] += e->timing[k];
    }
    for (int k = 0; k < 4; k++) e->timing[k] = sum[k];
    return DRNA_OK;
  };
  if (e->solo_left > 0) {             // after repeated lost partners: one workgroup per fold for a while
    const int rc = fold_solo(e, sub_batches);
    e->solo_left--;
    return rc;
  }
  return sub_batches();
}

// host-mapped E(targets) of max_R sequences against the installed targets (allocated on first use, again after more targets)
static int mapped_Ed(drna_engine* e) {
  const size_t cap = (size_t)e->max_R * (e->n_targets > 0 ? e->n_targets : 1);
  if (e->hm_Ed_cap >= cap) return DRNA_OK;
  if (e->hm_Ed) (void)hipHostFree(e->hm_Ed);
  e->hm_Ed = nullptr; e->hm_Ed_cap = 0;
  HIP_TRY(hipHostMalloc((void**)&e->hm_Ed, cap * sizeof(int32_t), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_Ed, e->hm_Ed, 0));
  e->hm_Ed_cap = cap;
  return DRNA_OK;
}

extern "C" int drna_score_batch(drna_engine* e, int R, int L, const char* seqs, uint32_t flags, double* Epf,
                                int32_t* Emfe, char* mfe_ss, int32_t* Ed) {
  if (!e) return DRNA_ERR_ARG;
  const bool want_pf = flags & DRNA_NEED_PF, want_mfe = flags & (DRNA_NEED_MFE | DRNA_NEED_PK),
             want_ev = flags & DRNA_NEED_EVAL;
  { const int rc = score_check(e, R, L, seqs, flags, Epf, Emfe, mfe_ss, Ed); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  const size_t ned = (size_t)R * (e->n_targets > 0 ? e->n_targets : 1);
  if (want_ev) { const int rc = mapped_Ed(e); if (rc != DRNA_OK) return rc; }
  std::memcpy(e->hm_seqs, seqs, (size_t)R * L);
  int rc = drna_score_batch_device(e, R, L, e->dm_seqs, flags, e->dm_Epf, e->dm_Emfe, e->dm_ss, e->dm_Ed);
  if (rc != DRNA_OK) return rc;
  if (want_pf) std::memcpy(Epf, e->hm_Epf, (size_t)R * sizeof(double));
  if (want_mfe) {
    std::memcpy(Emfe, e->hm_Emfe, (size_t)R * sizeof(int32_t));
    std::memcpy(mfe_ss, e->hm_ss, (size_t)R * L);
  }
  if (want_ev) std::memcpy(Ed, e->hm_Ed, ned * sizeof(int32_t));
  return DRNA_OK;
}

extern "C" int drna_last_timing(const drna_engine* e, float out[4]) {
  if (!e || !out) return DRNA_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = e->timing[k];
  return DRNA_OK;
}

extern "C" int drna_timing_sums(drna_engine* e, double out[5], int reset) {
  if (!e) return DRNA_ERR_ARG;
  if (out) for (int k = 0; k < 5; k++) out[k] = e->timing_sum[k];
  if (reset) for (int k = 0; k < 5; k++) e->timing_sum[k] = 0.0;
  return DRNA_OK;
}

extern "C" int drna_info(const drna_engine* e, int64_t out[6]) {
  if (!e || !out) return DRNA_ERR_ARG;
  out[0] = e->device; out[1] = e->max_R; out[2] = e->max_L; out[3] = 1024; out[4] = e->cus; out[5] = (int64_t)e->ws_bytes;
  return DRNA_OK;
}

// ---------------------------------------------------------------- auxiliary entry points: shared checks

// Argument check of the entry points beside the score_batch family; who names the entry point in the message.  R and L within the
// engine's limits, two strands (cut given) split inside the sequence, and ok: the required pointers (need says which) are there
static int aux_check(drna_engine* e, const char* who, int R, int L, const int* cut, bool ok, const char* need) {
  if (R >= 1 && R <= e->max_R && L >= 1 && L <= e->max_L && (!cut || (*cut >= 1 && *cut < L)) && ok) return DRNA_OK;
  e->err = std::string(who) + ": bad argument (R, L within the engine's limits" + (cut ? ", 1 <= cut < L; " : "; ") + need + ")";
  return DRNA_ERR_ARG;
}
static int need_targets(drna_engine* e, const char* who, int L) {
  if (e->n_targets >= 1 && e->L_targets == L) return DRNA_OK;
  e->err = std::string(who) + ": needs drna_set_targets() with the same L ('&' removed; targets[0] is the reference structure)";
  return DRNA_ERR_ARG;
}
static int fits_workspace(drna_engine* e, const char* who, int R) {
  if (R <= e->ws_slots) return DRNA_OK;
  e->err = std::string(who) + ": batch larger than the workspace (raise DRNA_WS_GB or split the batch)";
  return DRNA_ERR_ARG;
}

// ---------------------------------------------------------------- ensemble defect (inside + outside recursion), one and two strands

// workspace of the outside recursions (one strand: OB, OBI, A, CL and q5; two strands: the four tables without joining pairs),
// ws_slots sequences of max_L, allocated on first use
static int outside_workspace(drna_engine* e) {
  if (!e->d_ws_out) {
    const size_t b = (size_t)outside_ws_stride(e->max_L + 2) * sizeof(double) * e->ws_slots;
    HIP_TRY(hipMalloc((void**)&e->d_ws_out, b));
    e->ws_bytes += b;
  }
  return DRNA_OK;
}

// the inside kernel, then the outside kernel on its tables, both on the partition function's stream and timed (timing_edef);
// the R sequences are the caller's r_base, r_base + 1, ... or, with order (a ragged batch), status word q is that of the caller's order[q]
template <class Inside, class Outside>
static int inside_outside(drna_engine* e, int R, int r_base, const char* internal_msg, Inside&& inside, Outside&& outside,
                          const int* order = nullptr) {
  reset_status(e);
  HIP_TRY(hipEventRecord(e->ev_o0, e->s_pf));
  inside();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_o1, e->s_pf));
  outside();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_o2, e->s_pf));
  HIP_TRY(hipStreamSynchronize(e->s_pf));
  HIP_TRY(hipEventElapsedTime(&e->timing_edef[0], e->ev_o0, e->ev_o1));
  HIP_TRY(hipEventElapsedTime(&e->timing_edef[1], e->ev_o1, e->ev_o2));
  return fold_status(e, R, false, true, order, r_base, internal_msg);
}

// one batch that fits the workspaces; its sequences are the caller's r_base, r_base + 1, ...
static int ensemble_defect_impl(drna_engine* e, int R, int L, const char* d_seqs, double* d_edef, double* d_bpp, int r_base) {
  const int ld = L + 2;
  // the general inside kernel: it leaves qb / qm / qm1 in the workspace (the LDS kernel keeps only rings)
  PfArgs a = pf_args(e, d_seqs, L, ld, e->d_Epf);
  a.q5_stride = outside_ws_stride(ld);
  a.q5out = e->d_ws_out + (size_t)4 * ld * ld;
  OutArgs o;
  o.T = e->d_pfT; o.plan = e->d_plan; o.scale = e->d_scale; o.eMLb = e->d_eMLb;
  o.seqs = d_seqs; o.L = L; o.ld = ld;
  o.ws = e->d_ws_pf; o.ws_stride = a.ws_stride;
  o.wo = e->d_ws_out; o.wo_stride = outside_ws_stride(ld);
  o.pt = e->d_pt; o.edef = d_edef; o.bpp = d_bpp; o.pf_status = e->d_status + e->max_R;
  return inside_outside(e, R, r_base, "unexpected status of the partition function",
                        [&] { hipLaunchKernelGGL(pf_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, a); },
                        [&] { hipLaunchKernelGGL(outside_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, o); });
}
// two strands (cofold_pf_kernel, then the outside recursion on its tables); pairs r_base, r_base + 1, ...
static int cofold_edef_impl(drna_engine* e, int R, int L, int cut, const char* d_seqs, double* d_edef, double* d_bpp, int r_base) {
  const int ld = L + 2;
  const CoArgs a = co_args(e, d_seqs, L, cut, ld);
  CoOutArgs o;
  o.F = e->d_pfT; o.plan = e->d_plan; o.scale = e->d_scale; o.eMLb = e->d_eMLb;
  o.seqs = d_seqs; o.L = L; o.cut = cut; o.ld = ld; o.eDuplexInit = a.eDuplexInit;
  o.wsp = e->d_ws_pf; o.wsp_stride = a.wsp_stride;         // the four outside tables fill the slot behind QB, QM, QM1, INFO
  o.wu = e->d_ws_out; o.wu_stride = outside_ws_stride(ld);
  o.pt = e->d_pt; o.edef = d_edef; o.bpp = d_bpp; o.status_pf = a.status_pf;
  return inside_outside(e, R, r_base, "unexpected status of the co-fold partition function",
                        [&] { hipLaunchKernelGGL(cofold_pf_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, a); },
                        [&] { hipLaunchKernelGGL(cofold_outside_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, o); });
}

// short designs: inside and outside sweep in one launch on tables in LDS (fold_edef_lds.hpp), no workspace slot; cut = 0: one
// strand, the instance with an empty second strand.  timing_edef[0] is the launch, [1] stays ~0
static int edef_lds_impl(drna_engine* e, int R, int L, int cut, const char* d_seqs, double* d_edef, double* d_bpp, int r_base) {
  EdefLdsArgs a;
  a.in = co_args(e, d_seqs, L, cut ? cut : L, 0);
  a.out.F = e->d_pfT; a.out.plan = e->d_plan; a.out.scale = e->d_scale; a.out.eMLb = e->d_eMLb;
  a.out.seqs = d_seqs; a.out.L = L; a.out.cut = a.in.cut; a.out.eDuplexInit = a.in.eDuplexInit;
  a.out.pt = e->d_pt; a.out.edef = d_edef; a.out.bpp = d_bpp; a.out.status_pf = a.in.status_pf;
  e->edef_lds_calls++;
  return inside_outside(e, R, r_base, "unexpected status of the ensemble-defect kernel",
                        [&] {
                          if (cut) hipLaunchKernelGGL((edef_lds_kernel<1024, false>), dim3(R), dim3(1024), 0, e->s_pf, a);
                          else hipLaunchKernelGGL((edef_lds_kernel<1024, true>), dim3(R), dim3(1024), 0, e->s_pf, a);
                        },
                        [] {});
}

// R sequences in device memory (cut = 0: one strand), the caller's r_base, r_base + 1, ...  Short ones take the fused LDS kernel
// (option "edef_lds"), in chunks of max_R (the status words); the others one sub-batch of ws_slots after the other (the
// workspaces, DRNA_WS_GB).  last_edef_timing = the chunks' sums, added to *tsum when given
static int edef_batch_device(drna_engine* e, int R, int L, int cut, const char* d_seqs, double* d_edef, double* d_bpp, int r_base = 0,
                             float* tsum = nullptr) {
  static_assert(sizeof(double) == 8, "workspace strides are counted in doubles");
  const bool lds = e->edef_lds && L <= (cut ? CO_EDEF_LDS_MAX : EDEF_LDS_HOST_MAX);
  if (!lds && cut && (cofold_outside_ws_stride(L + 2) > (long long)pf_ws_stride(L + 2) || 4ll * (L + 2) * (L + 2) > outside_ws_stride(L + 2))) {
    e->err = "drna_cofold_ensemble_defect_batch: workspace slot too small for the outside tables";
    return DRNA_ERR_INTERNAL;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (!lds) { const int rc = outside_workspace(e); if (rc != DRNA_OK) return rc; }
  if ((cut || lds) && !e->d_F4) HIP_TRY(hipMalloc((void**)&e->d_F4, (size_t)4 * e->max_R * sizeof(double)));
  float sum[2] = {0, 0};
  const int step = lds ? e->max_R : e->ws_slots;
  for (int r0 = 0; r0 < R; r0 += step) {
    const int m = std::min(step, R - r0);
    const char* s = d_seqs + (size_t)r0 * L;
    double* b = d_bpp ? d_bpp + (size_t)r0 * (L + 1) * (L + 1) : nullptr;
    const int rc = lds   ? edef_lds_impl(e, m, L, cut, s, d_edef + r0, b, r_base + r0)
                   : cut ? cofold_edef_impl(e, m, L, cut, s, d_edef + r0, b, r_base + r0)
                         : ensemble_defect_impl(e, m, L, s, d_edef + r0, b, r_base + r0);
    if (rc != DRNA_OK) return rc;
    sum[0] += e->timing_edef[0]; sum[1] += e->timing_edef[1];
  }
  e->timing_edef[0] = sum[0]; e->timing_edef[1] = sum[1];
  if (tsum) { tsum[0] += sum[0]; tsum[1] += sum[1]; }
  return DRNA_OK;
}

// the same from and to host memory; bpp optional.  R is not limited by max_R: the staging buffers take max_R sequences at a time
static int edef_batch_host(drna_engine* e, int R, int L, int cut, const char* seqs, double* edef, double* bpp) {
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_edef) HIP_TRY(hipMalloc((void**)&e->d_edef, (size_t)e->max_R * sizeof(double)));
  double* d_bpp = nullptr;
  const size_t nb = (size_t)R * (L + 1) * (L + 1) * sizeof(double);
  if (bpp) {
    HIP_TRY(hipMalloc((void**)&d_bpp, nb));
    hipError_t z = hipMemset(d_bpp, 0, nb);
    if (z == hipSuccess) z = hipDeviceSynchronize();     // the memset runs on the null stream, the kernels on a non-blocking stream
    if (z != hipSuccess) { (void)hipFree(d_bpp); e->err = "hipMemset(bpp)"; return DRNA_ERR_DEVICE; }
  }
  int rc = DRNA_OK;
  float sum[2] = {0, 0};
  for (int r0 = 0; r0 < R && rc == DRNA_OK; r0 += e->max_R) {
    const int m = std::min(e->max_R, R - r0);
    if (hipMemcpy(e->d_seqs, seqs + (size_t)r0 * L, (size_t)m * L, hipMemcpyHostToDevice) != hipSuccess) { e->err = "hipMemcpy(seqs)"; rc = DRNA_ERR_DEVICE; break; }
    rc = edef_batch_device(e, m, L, cut, e->d_seqs, e->d_edef, d_bpp ? d_bpp + (size_t)r0 * (L + 1) * (L + 1) : nullptr, r0, sum);
    if (rc == DRNA_OK && hipMemcpy(edef + r0, e->d_edef, (size_t)m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { e->err = "hipMemcpy(edef)"; rc = DRNA_ERR_DEVICE; }
  }
  e->timing_edef[0] = sum[0]; e->timing_edef[1] = sum[1];
  if (rc == DRNA_OK && bpp && hipMemcpy(bpp, d_bpp, nb, hipMemcpyDeviceToHost) != hipSuccess) { e->err = "hipMemcpy(bpp)"; rc = DRNA_ERR_DEVICE; }
  if (d_bpp) (void)hipFree(d_bpp);
  return rc;
}

// (R >= 1 is all that is asked of R: a batch beyond max_R goes through the staging buffers and status words in chunks)
static int edef_check(drna_engine* e, const char* who, int R, int L, const int* cut, bool ok) {
  const int rc = aux_check(e, who, std::min(R, e->max_R), L, cut, ok, "seqs and edef required");
  return rc != DRNA_OK ? rc : need_targets(e, who, L);
}

extern "C" int drna_ensemble_defect_batch_device(drna_engine* e, int R, int L, const char* d_seqs, double* d_edef,
                                                 double* d_bpp) {
  if (!e) return DRNA_ERR_ARG;
  const int rc = edef_check(e, "drna_ensemble_defect_batch", R, L, nullptr, d_seqs && d_edef);
  return rc != DRNA_OK ? rc : edef_batch_device(e, R, L, 0, d_seqs, d_edef, d_bpp);
}

extern "C" int drna_ensemble_defect_batch(drna_engine* e, int R, int L, const char* seqs, double* edef, double* bpp) {
  if (!e) return DRNA_ERR_ARG;
  const int rc = edef_check(e, "drna_ensemble_defect_batch", R, L, nullptr, seqs && edef);
  return rc != DRNA_OK ? rc : edef_batch_host(e, R, L, 0, seqs, edef, bpp);
}

extern "C" int drna_cofold_ensemble_defect_batch(drna_engine* e, int R, int L, int cut, const char* seqs, double* edef, double* bpp) {
  if (!e) return DRNA_ERR_ARG;
  const int rc = edef_check(e, "drna_cofold_ensemble_defect_batch", R, L, &cut, seqs && edef);
  return rc != DRNA_OK ? rc : edef_batch_host(e, R, L, cut, seqs, edef, bpp);
}

extern "C" int drna_last_edef_timing(const drna_engine* e, float out[2]) {
  if (!e || !out) return DRNA_ERR_ARG;
  out[0] = e->timing_edef[0]; out[1] = e->timing_edef[1];
  return DRNA_OK;
}

// ---------------------------------------------------------------- stochastic traceback (fold_sample.hpp)

constexpr int SAMPLE_NT = 256;      // four waves, i.e. four samples in flight per workgroup (56 KB of LDS: two workgroups per CU)

// m sequences that fit the workspaces (the caller's r_base, r_base + 1, ...): pf_kernel, then sample_kernel on its tables, both on
// the partition function's stream and timed as the ensemble defect's two launches are (timing_edef).  G workgroups per sequence so
// that the chip is covered twice over (a wave takes the samples of its stride one after the other).
static int sample_impl(drna_engine* e, int m, int L, int S, const char* d_seqs, const uint64_t* d_seeds, char* d_ss, int32_t* d_E,
                       int r_base) {
  const int ld = L + 2;
  SampleArgs a{};
  a.pf = pf_args(e, d_seqs, L, ld, e->d_Epf);
  a.pf.q5out = e->d_q5s; a.pf.q5_stride = ld;
  a.ev = eval_args(e, d_seqs, L, nullptr);
  a.seeds = d_seeds; a.S = S; a.ss = d_ss; a.E = d_E;
  constexpr int NW = SAMPLE_NT / WAVE;
  a.G = std::max(1, std::min((S + NW - 1) / NW, (4 * e->cus + m - 1) / m));
  e->sample_calls++;
  return inside_outside(e, m, r_base, "unexpected status of the partition function",
                        [&] { hipLaunchKernelGGL(pf_kernel<1024>, dim3(m), dim3(1024), 0, e->s_pf, a.pf); },
                        [&] { hipLaunchKernelGGL(sample_kernel<SAMPLE_NT>, dim3(m * a.G), dim3(SAMPLE_NT), 0, e->s_pf, a); });
}

// two strands: cofold_pf_kernel (always the workspace instance: the LDS instance leaves no tables), then the columns launch and
// cofold_sample_kernel on its tables; pairs r_base, r_base + 1, ...
static int cofold_sample_impl(drna_engine* e, int m, int L, int cut, int S, const char* d_seqs, const uint64_t* d_seeds, char* d_ss,
                              int32_t* d_E, int r_base) {
  CoSampleArgs a{};
  a.co = co_args(e, d_seqs, L, cut, L + 2);
  a.ev = eval_args(e, d_seqs, L, nullptr);
  a.ev.cut = cut; a.ev.DuplexInit = e->H.DuplexInit;
  a.cols = e->d_cocols; a.col_stride = e->max_L + 2;
  a.seeds = d_seeds; a.S = S; a.ss = d_ss; a.E = d_E;
  constexpr int NW = SAMPLE_NT / WAVE;
  a.G = std::max(1, std::min((S + NW - 1) / NW, (4 * e->cus + m - 1) / m));
  e->cofold_sample_calls++;
  return inside_outside(e, m, r_base, "unexpected status of the co-fold partition function",
                        [&] { hipLaunchKernelGGL(cofold_pf_kernel<1024>, dim3(m), dim3(1024), 0, e->s_pf, a.co); },
                        [&] {
                          hipLaunchKernelGGL(cofold_columns_kernel<256>, dim3(m), dim3(256), 0, e->s_pf, a);
                          hipLaunchKernelGGL(cofold_sample_kernel<SAMPLE_NT>, dim3(m * a.G), dim3(SAMPLE_NT), 0, e->s_pf, a);
                        });
}

// The sample buffers of a call and its chunks of the workspace slots (and of max_R: the staging buffer and the status words).
// impl(m, d_seeds, d_ss, d_E, r0) folds and samples the m sequences (pairs) of a chunk from e->d_seqs; extra(m, r0) copies out what
// else the entry point returns per sequence.  last_edef_timing = the chunks' sums
template <class Impl, class Extra>
static int sample_chunks(drna_engine* e, int R, int L, const char* seqs, int S, const uint64_t* seeds, char* ss, int32_t* E,
                         uint64_t* d_seeds, char* d_ss, int32_t* d_E, int step, Impl&& impl, Extra&& extra) {
  float sum[2] = {0, 0};
  for (int r0 = 0; r0 < R; r0 += step) {
    const int m = std::min(step, R - r0);
    const size_t cells = (size_t)m * S;
    HIP_TRY(hipMemcpy(e->d_seqs, seqs + (size_t)r0 * L, (size_t)m * L, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seeds, seeds + r0, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice));
    int rc = impl(m, d_seeds, d_ss, E ? d_E : nullptr, r0);
    if (rc != DRNA_OK) return rc;
    sum[0] += e->timing_edef[0]; sum[1] += e->timing_edef[1];
    HIP_TRY(hipMemcpy(ss + (size_t)r0 * S * L, d_ss, cells * L, hipMemcpyDeviceToHost));
    if (E) HIP_TRY(hipMemcpy(E + (size_t)r0 * S, d_E, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    rc = extra(m, r0);
    if (rc != DRNA_OK) return rc;
  }
  e->timing_edef[0] = sum[0]; e->timing_edef[1] = sum[1];
  return DRNA_OK;
}
template <class Impl, class Extra>
static int sample_batch_host(drna_engine* e, const char* who, int R, int L, const char* seqs, int S, const uint64_t* seeds, char* ss,
                             int32_t* E, Impl&& impl, Extra&& extra) {
  const int step = std::min(std::min(e->ws_slots, e->max_R), R);
  uint64_t* d_seeds = nullptr;
  char* d_ss = nullptr;
  int32_t* d_E = nullptr;
  int rc = DRNA_OK;
  if (hipMalloc((void**)&d_seeds, (size_t)step * sizeof(uint64_t)) != hipSuccess ||
      hipMalloc((void**)&d_ss, (size_t)step * S * L) != hipSuccess ||
      hipMalloc((void**)&d_E, (size_t)step * S * sizeof(int32_t)) != hipSuccess) {
    e->err = std::string(who) + ": hipMalloc of the sample buffers failed";
    rc = DRNA_ERR_DEVICE;
  }
  if (rc == DRNA_OK) rc = sample_chunks(e, R, L, seqs, S, seeds, ss, E, d_seeds, d_ss, d_E, step, impl, extra);
  if (d_seeds) (void)hipFree(d_seeds);
  if (d_ss) (void)hipFree(d_ss);
  if (d_E) (void)hipFree(d_E);
  return rc;
}
// the argument errors of both sample entry points (cut: two strands)
static int sample_check(drna_engine* e, const char* who, int R, int L, const int* cut, int S, bool ptrs) {
  const int rc = aux_check(e, who, std::min(R, e->max_R), L, cut, S >= 1 && ptrs, "S >= 1; seqs, seeds and ss required");
  if (rc != DRNA_OK) return rc;
  if ((long long)R * S > (long long)DRNA_SAMPLE_MAX_CHARS / L) {
    e->err = std::string(who) + ": R x S x L above DRNA_SAMPLE_MAX_CHARS";
    return DRNA_ERR_ARG;
  }
  return DRNA_OK;
}
// a per-slot buffer of the samplers, allocated on first use: per_slot doubles for each of the ws_slots sequences
static int sample_columns(drna_engine* e, double** buf, size_t per_slot) {
  if (*buf) return DRNA_OK;
  const size_t b = (size_t)e->ws_slots * per_slot * sizeof(double);
  HIP_TRY(hipMalloc((void**)buf, b));
  e->ws_bytes += b;
  return DRNA_OK;
}

extern "C" int drna_sample_structures_batch(drna_engine* e, int R, int L, const char* seqs, int S, const uint64_t* seeds, char* ss,
                                            int32_t* E, double* Epf) {
  if (!e) return DRNA_ERR_ARG;
  const char* who = "drna_sample_structures_batch";
  { const int rc = sample_check(e, who, R, L, nullptr, S, seqs && seeds && ss); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  { const int rc = sample_columns(e, &e->d_q5s, (size_t)e->max_L + 2); if (rc != DRNA_OK) return rc; }
  return sample_batch_host(
      e, who, R, L, seqs, S, seeds, ss, E,
      [&](int m, const uint64_t* d_seeds, char* d_ss, int32_t* d_E, int r0) -> int { return sample_impl(e, m, L, S, e->d_seqs, d_seeds, d_ss, d_E, r0); },
      [&](int m, int r0) -> int {
        if (Epf) HIP_TRY(hipMemcpy(Epf + r0, e->d_Epf, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
        return DRNA_OK;
      });
}

extern "C" int drna_cofold_sample_structures_batch(drna_engine* e, int R, int L, int cut, const char* seqs, int S, const uint64_t* seeds,
                                                   char* ss, int32_t* E, double* F4) {
  if (!e) return DRNA_ERR_ARG;
  const char* who = "drna_cofold_sample_structures_batch";
  { const int rc = sample_check(e, who, R, L, &cut, S, seqs && seeds && ss); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  { const int rc = sample_columns(e, &e->d_cocols, (size_t)CO_COLS * (e->max_L + 2)); if (rc != DRNA_OK) return rc; }
  if (!e->d_F4) HIP_TRY(hipMalloc((void**)&e->d_F4, (size_t)4 * e->max_R * sizeof(double)));
  return sample_batch_host(
      e, who, R, L, seqs, S, seeds, ss, E,
      [&](int m, const uint64_t* d_seeds, char* d_ss, int32_t* d_E, int r0) -> int { return cofold_sample_impl(e, m, L, cut, S, e->d_seqs, d_seeds, d_ss, d_E, r0); },
      [&](int m, int r0) -> int {
        if (F4) HIP_TRY(hipMemcpy(F4 + (size_t)4 * r0, e->d_F4, (size_t)4 * m * sizeof(double), hipMemcpyDeviceToHost));
        return DRNA_OK;
      });
}

// ---------------------------------------------------------------- MEA and centroid structures (fold_mea.hpp)

constexpr int MEA_NT = 512;         // 64 cells of a diagonal at a time (MEA_GW lanes each)

// the device buffers of one call: the chunk's pair probabilities and what mea_kernel returns per sequence
struct MeaBuffers {
  double *bpp = nullptr, *val = nullptr, *dist = nullptr;
  char *mss = nullptr, *css = nullptr;
  int32_t *E = nullptr, *nc = nullptr;
  ~MeaBuffers() {
    for (void* p : {(void*)bpp, (void*)val, (void*)dist, (void*)mss, (void*)css, (void*)E, (void*)nc})
      if (p) (void)hipFree(p);
  }
};

// mea_kernel on the m matrices of a chunk (timed: timing_mea[2] grows by the launch); the stream is idle before and after
static int mea_launch(drna_engine* e, int m, int L, int cut, double gamma, const MeaBuffers& b, bool want_E) {
  MeaArgs a;
  a.ev = eval_args(e, e->d_seqs, L, nullptr);
  a.ev.cut = cut; a.ev.DuplexInit = cut ? e->H.DuplexInit : 0;
  a.bpp = b.bpp; a.ws = e->d_ws_out; a.ws_stride = outside_ws_stride(L + 2); a.gamma = gamma;
  a.mea_ss = b.mss; a.mea_val = b.val; a.cen_ss = b.css; a.cen_dist = b.dist; a.E = want_E ? b.E : nullptr; a.ncand = b.nc;
  e->mea_calls++;
  HIP_TRY(hipEventRecord(e->ev_o0, e->s_pf));
  if (e->mea_lds && L <= MEA_LDS_MAX) hipLaunchKernelGGL((mea_kernel<MEA_NT, true>), dim3(m), dim3(MEA_NT), 0, e->s_pf, a);
  else hipLaunchKernelGGL((mea_kernel<MEA_NT, false>), dim3(m), dim3(MEA_NT), 0, e->s_pf, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_o1, e->s_pf));
  HIP_TRY(hipStreamSynchronize(e->s_pf));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e->ev_o0, e->ev_o1));
  e->timing_mea[2] += ms;
  return DRNA_OK;
}

// the chunks of a call: inside and outside pass by edef_batch_device against the all-unpaired pair table (its edef is dropped),
// then mea_kernel on the chunk's matrices
static int mea_chunks(drna_engine* e, int R, int L, int cut, const char* seqs, double gamma, char* mea_ss, double* mea_val,
                      char* cen_ss, double* cen_dist, int32_t* E, double* bpp, int step, const MeaBuffers& b) {
  const size_t cells = (size_t)(L + 1) * (L + 1);
  std::vector<int32_t> nc(step);
  for (int r0 = 0; r0 < R; r0 += step) {
    const int m = std::min(step, R - r0);
    HIP_TRY(hipMemcpy(e->d_seqs, seqs + (size_t)r0 * L, (size_t)m * L, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(b.bpp, 0, (size_t)m * cells * sizeof(double), e->s_pf));     // the outside pass writes the pairs only
    float t[2] = {0, 0};
    int rc = edef_batch_device(e, m, L, cut, e->d_seqs, e->d_edef, b.bpp, r0, t);
    if (rc != DRNA_OK) return rc;
    e->timing_mea[0] += t[0]; e->timing_mea[1] += t[1];
    rc = mea_launch(e, m, L, cut, gamma, b, E != nullptr);
    if (rc != DRNA_OK) return rc;
    HIP_TRY(hipMemcpy(mea_ss + (size_t)r0 * L, b.mss, (size_t)m * L, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cen_ss + (size_t)r0 * L, b.css, (size_t)m * L, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mea_val + r0, b.val, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cen_dist + r0, b.dist, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (E) HIP_TRY(hipMemcpy(E + 2 * (size_t)r0, b.E, 2 * (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (bpp) HIP_TRY(hipMemcpy(bpp + (size_t)r0 * cells, b.bpp, (size_t)m * cells * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nc.data(), b.nc, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int q = 0; q < m; q++) e->mea_cands = (int)std::min<long long>((long long)e->mea_cands + nc[q], 0x7fffffff);
  }
  return DRNA_OK;
}

// cut = 0: one strand.  Needs no installed targets and leaves them alone
static int mea_batch_host(drna_engine* e, const char* who, int R, int L, int cut, const char* seqs, double gamma, char* mea_ss,
                          double* mea_val, char* cen_ss, double* cen_dist, int32_t* E, double* bpp) {
  {
    const bool ok = gamma > 0.0 && std::isfinite(gamma) && seqs && mea_ss && mea_val && cen_ss && cen_dist;
    const int rc = aux_check(e, who, std::min(R, e->max_R), L, cut ? &cut : nullptr, ok,
                             "gamma > 0 and finite; seqs, mea_ss, mea_val, cen_ss and cen_dist required");
    if (rc != DRNA_OK) return rc;
  }
  // a failed call leaves zeros
  memset(mea_ss, 0, (size_t)R * L); memset(cen_ss, 0, (size_t)R * L);
  std::fill(mea_val, mea_val + R, 0.0); std::fill(cen_dist, cen_dist + R, 0.0);
  if (E) std::fill(E, E + 2 * (size_t)R, 0);
  HIP_TRY(hipSetDevice(e->device));
  { const int rc = outside_workspace(e); if (rc != DRNA_OK) return rc; }      // M beyond MEA_LDS_MAX, candidate lists beyond MEA_CAND_LDS
  if (3ll * (L + 2) * (L + 2) > outside_ws_stride(L + 2)) { e->err = std::string(who) + ": workspace slot too small"; return DRNA_ERR_INTERNAL; }
  if (!e->d_edef) HIP_TRY(hipMalloc((void**)&e->d_edef, (size_t)e->max_R * sizeof(double)));
  if (!e->d_mea_pt) {
    HIP_TRY(hipMalloc((void**)&e->d_mea_pt, (size_t)(e->max_L + 2) * sizeof(short)));
    HIP_TRY(hipMemset(e->d_mea_pt, 0, (size_t)(e->max_L + 2) * sizeof(short)));
    HIP_TRY(hipDeviceSynchronize());
  }
  const int step = std::min(std::min(e->ws_slots, e->max_R), R);
  const size_t cells = (size_t)(L + 1) * (L + 1);
  MeaBuffers b;
  if (hipMalloc((void**)&b.bpp, (size_t)step * cells * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&b.val, (size_t)step * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&b.dist, (size_t)step * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&b.mss, (size_t)step * L) != hipSuccess || hipMalloc((void**)&b.css, (size_t)step * L) != hipSuccess ||
      hipMalloc((void**)&b.E, 2 * (size_t)step * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&b.nc, (size_t)step * sizeof(int32_t)) != hipSuccess) {
    e->err = std::string(who) + ": hipMalloc of the call's buffers failed";
    return DRNA_ERR_DEVICE;
  }
  e->timing_mea[0] = e->timing_mea[1] = e->timing_mea[2] = 0;
  e->mea_cands = 0;
  short* const installed = e->d_pt;
  e->d_pt = e->d_mea_pt;
  const int rc = mea_chunks(e, R, L, cut, seqs, gamma, mea_ss, mea_val, cen_ss, cen_dist, E, bpp, step, b);
  e->d_pt = installed;
  return rc;
}

extern "C" int drna_mea_structures_batch(drna_engine* e, int R, int L, const char* seqs, double gamma, char* mea_ss, double* mea_val,
                                         char* cen_ss, double* cen_dist, int32_t* E, double* bpp) {
  if (!e) return DRNA_ERR_ARG;
  return mea_batch_host(e, "drna_mea_structures_batch", R, L, 0, seqs, gamma, mea_ss, mea_val, cen_ss, cen_dist, E, bpp);
}

extern "C" int drna_cofold_mea_structures_batch(drna_engine* e, int R, int L, int cut, const char* seqs, double gamma, char* mea_ss,
                                                double* mea_val, char* cen_ss, double* cen_dist, int32_t* E, double* bpp) {
  if (!e) return DRNA_ERR_ARG;
  if (cut < 1 || cut >= L) { e->err = "drna_cofold_mea_structures_batch: bad argument (1 <= cut < L)"; return DRNA_ERR_ARG; }
  return mea_batch_host(e, "drna_cofold_mea_structures_batch", R, L, cut, seqs, gamma, mea_ss, mea_val, cen_ss, cen_dist, E, bpp);
}

extern "C" int drna_last_mea_timing(const drna_engine* e, float out[3]) {
  if (!e || !out) return DRNA_ERR_ARG;
  for (int k = 0; k < 3; k++) out[k] = e->timing_mea[k];
  return DRNA_OK;
}

// ---------------------------------------------------------------- ragged batches (sequences of different lengths)

extern "C" int drna_set_targets_ragged(drna_engine* e, int n_targets, const int32_t* lens, const char* targets) {
  if (!e) return DRNA_ERR_ARG;
  if (n_targets < 1 || !lens || !targets) { e->err = "drna_set_targets_ragged: bad argument"; return DRNA_ERR_ARG; }
  std::vector<int> off(n_targets);
  size_t total = 0, chars = 0;
  for (int t = 0; t < n_targets; t++) {
    if (lens[t] < 1 || lens[t] > e->max_L) { e->err = "drna_set_targets_ragged: structure length outside [1, max_L]"; return DRNA_ERR_ARG; }
    off[t] = (int)total;
    total += (size_t)lens[t] + 2;
  }
  std::vector<short> pt(total, 0);
  for (int t = 0; t < n_targets; t++) {
    const int rc = target_pairs(e, "drna_set_targets_ragged", targets + chars, lens[t], pt.data() + off[t]);
    if (rc != DRNA_OK) return rc;
    chars += (size_t)lens[t];
  }
  HIP_TRY(hipSetDevice(e->device));
  if (e->d_rpt) { (void)hipFree(e->d_rpt); e->d_rpt = nullptr; }
  if (e->d_rpt_off) { (void)hipFree(e->d_rpt_off); e->d_rpt_off = nullptr; }
  HIP_TRY(upload(&e->d_rpt, pt.data(), pt.size()));
  HIP_TRY(upload(&e->d_rpt_off, off.data(), off.size()));
  e->rt_len.assign(lens, lens + n_targets);
  return DRNA_OK;
}

// One fold of a ragged batch of R sequences sorted longest first (lengths h[q]), in chunks of ws_slots consecutive positions q:
// per chunk the strip kernels take idxC (one launch per number of strips, most strips first), the general kernel idxD, the LDS-
// resident kernel idxA.  set_chunk(c0) points the fold's arguments at the chunk's workspace; a launch gets the number of its
// sequences and their index list on the device, in the plan's descriptor block d_rg (a strip launch also the number of strips and
// the first flag slot).
template <class SetChunk, class Strips, class General, class Lds>
static void ragged_fold(drna_engine* e, int R, const int* h, const int* idxA, int nA, const int* idxC, int nC, const int* idxD, int nD,
                        const int* d_rg, SetChunk&& set_chunk, Strips&& launch_strips, General&& launch_general, Lds&& launch_lds) {
  const int ld = e->max_L + 2;
  // first entry of an index list (ascending q) that is not below q: the list's part in the chunk [c0, c1) is [lo(c0), lo(c1))
  auto lo = [](const int* idx, int cnt, int q) { return (int)(std::lower_bound(idx, idx + cnt, q) - idx); };
  for (int c0 = 0; c0 < R; c0 += e->ws_slots) {
    const int c1 = std::min(R, c0 + e->ws_slots);
    set_chunk(c0);
    for (int k = lo(idxC, nC, c0), end = lo(idxC, nC, c1); k < end;) {
      const int S = strips_for(e, h[idxC[k]], ld);
      int k2 = k;
      while (k2 < end && strips_for(e, h[idxC[k2]], ld) == S) k2++;
      launch_strips(k2 - k, S, k, d_rg + (size_t)5 * R + k);
      k = k2;
    }
    const int fD = lo(idxD, nD, c0), mD = lo(idxD, nD, c1) - fD, fA = lo(idxA, nA, c0), mA = lo(idxA, nA, c1) - fA;
    if (mD) launch_general(mD, d_rg + (size_t)6 * R + fD);
    if (mA) launch_lds(mA, d_rg + (size_t)3 * R + fA);
  }
}
// R results of the sorted order back from the device into the caller's order
template <class T>
static int scatter_back(drna_engine* e, const T* d_src, const std::vector<int>& order, T* out) {
  std::vector<T> t(order.size());
  HIP_TRY(hipMemcpy(t.data(), d_src, t.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t q = 0; q < t.size(); q++) out[order[q]] = t[q];
  return DRNA_OK;
}

// What a ragged batch keeps from call to call while its lengths stay: drna_score_ragged plans and runs once, drna_mc_run_ragged
// plans once and runs every iteration.
// The batch is folded in SORTED order, longest first: position q on the device is sequence order[q] of the caller.  Then
// (a) the three classes -- strips (n > 200), general kernels, LDS-resident kernels (n <= 200) -- are ranges of q, and (b) a
// batch larger than the workspaces (ws_slots sequences, DRNA_WS_GB) goes through them in CHUNKS of consecutive q: chunk c
// uses slot q - c0, i.e. a workspace pointer moved back by c0 slots, its launches queue behind the previous chunk's on the
// same streams (the MFE stream owns the MFE workspace, the partition-function stream the other), and nothing waits in between.
// descriptors h: len | off | target_of | index lists (q values) of the LDS-resident kernels | - | strip kernels | general kernels
struct RaggedPlan {
  int R = 0, nA = 0, nC = 0, nD = 0, strips = 0;   // strips: the option "strips" the index lists were made under (fold_solo turns it off)
  uint32_t flags = 0;
  size_t total = 0;
  std::vector<int> order, h;
  std::vector<size_t> src_off;                     // of the caller's sequence r
  std::vector<char> sorted;                        // the sequences going up / the structures coming back, in sorted order
  int* d_rg = nullptr;                             // the plan's descriptor block on the device (rg_block)
};
// the descriptor blocks: the scoring plan's, the ensemble-defect plan's, the second-best fold's
enum : int { RG_SCORE = 0, RG_EDEF = 1, RG_SUB = 2, RG_BLOCKS = 3 };
static int rg_block(drna_engine* e, int which, int** out) {
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_rg) HIP_TRY(hipMalloc((void**)&e->d_rg, (size_t)RG_BLOCKS * 7 * e->max_R * sizeof(int)));
  *out = e->d_rg + (size_t)which * 7 * e->max_R;
  return DRNA_OK;
}
// the indices 0 .. order.size() - 1 by length, longest first (stable: equal lengths keep the caller's order)
static void longest_first(std::vector<int>& order, const int32_t* lens) {
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });
}
// the three kernel classes of the plan's lengths under the engine's strip option, and the descriptor block on the device
static int ragged_classes(drna_engine* e, RaggedPlan& p) {
  const int R = p.R, ld = e->max_L + 2;
  int *idxA = p.h.data() + (size_t)3 * R, *idxC = p.h.data() + (size_t)5 * R, *idxD = p.h.data() + (size_t)6 * R;
  p.nA = p.nC = p.nD = 0;
  for (int q = 0; q < R; q++) {
    const int len = p.h[q];
    if (len <= MFE_FAST_NMAX && len <= PF_FAST_NMAX) idxA[p.nA++] = q;
    else if (strips_for(e, len, ld) && len > PF_FAST_NMAX) idxC[p.nC++] = q;
    else idxD[p.nD++] = q;
  }
  p.strips = e->strips;
  { const int rc = rg_block(e, RG_SCORE, &p.d_rg); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipMemcpy(p.d_rg, p.h.data(), p.h.size() * sizeof(int), hipMemcpyHostToDevice));
  return DRNA_OK;
}
// the checks of a ragged batch (who names the entry point in the message), its sorted order (longest first) and the descriptors
// len | off | target_of; the index lists behind them are the caller's
static int ragged_layout(drna_engine* e, const char* who, int R, const int32_t* lens, const int32_t* target_of, uint32_t flags,
                         RaggedPlan& p) {
  const bool want_ev = flags & DRNA_NEED_EVAL;
  p.R = R; p.flags = flags; p.total = 0;
  p.order.resize(R);
  for (int r = 0; r < R; r++) {
    if (lens[r] < 1 || lens[r] > e->max_L) { e->err = std::string(who) + ": sequence length outside [1, max_L]"; return DRNA_ERR_ARG; }
    p.total += (size_t)lens[r];
    if (want_ev) {
      const int t = target_of[r];
      if (t < 0 || t >= (int)e->rt_len.size() || e->rt_len[t] != lens[r]) {
        e->err = std::string(who) + ": target_of[r] must name a structure of drna_set_targets_ragged() with the sequence's length";
        return DRNA_ERR_ARG;
      }
    }
  }
  if (p.total > (size_t)e->max_R * e->max_L) { e->err = std::string(who) + ": more nucleotides than max_R * max_L"; return DRNA_ERR_ARG; }
  longest_first(p.order, lens);
  p.src_off.resize(R);
  { size_t o = 0; for (int r = 0; r < R; r++) { p.src_off[r] = o; o += (size_t)lens[r]; } }
  p.h.assign((size_t)7 * R, 0);
  p.sorted.resize(p.total);
  size_t o = 0;
  for (int q = 0; q < R; q++) {
    const int r = p.order[q];
    p.h[q] = lens[r];
    p.h[(size_t)R + q] = (int)o;
    o += (size_t)lens[r];
    if (want_ev) p.h[(size_t)2 * R + q] = target_of[r];
  }
  return DRNA_OK;
}
static int ragged_plan(drna_engine* e, int R, const int32_t* lens, const int32_t* target_of, uint32_t flags, RaggedPlan& p) {
  { const int rc = ragged_layout(e, "drna_score_ragged", R, lens, target_of, flags, p); if (rc != DRNA_OK) return rc; }
  const bool want_ev = flags & DRNA_NEED_EVAL;
  { const int rc = ragged_classes(e, p); if (rc != DRNA_OK) return rc; }
  if (want_ev && !e->d_Ed) HIP_TRY(hipMalloc((void**)&e->d_Ed, (size_t)e->max_R * std::max(1, e->n_targets) * sizeof(int32_t)));
  return DRNA_OK;
}

// One scoring of the plan's batch: the sequences up, the launches, the status words, the results back in the caller's order
static int ragged_run(drna_engine* e, RaggedPlan& p, const char* seqs, double* Epf, int32_t* Emfe, char* mfe_ss, int32_t* Ed) {
  const uint32_t flags = p.flags;
  const bool want_pf = flags & DRNA_NEED_PF, want_mfe = flags & (DRNA_NEED_MFE | DRNA_NEED_PK),
             want_pk = flags & DRNA_NEED_PK, want_ev = flags & DRNA_NEED_EVAL;
  const int R = p.R;
  e->cur_with_pf = want_pf;
  auto again = [&] { return ragged_run(e, p, seqs, Epf, Emfe, mfe_ss, Ed); };
  if (!e->in_fallback && e->solo_left > 0) {             // (see drna_score_batch_device)
    const int rc = fold_solo(e, again);
    e->solo_left--;
    return rc;
  }
  if (p.strips != e->strips) { const int rc = ragged_classes(e, p); if (rc != DRNA_OK) return rc; }   // (a redone call, or the first after one)
  const int *h = p.h.data(), *off = h + R;
  const int *idxA = h + (size_t)3 * R, *idxC = h + (size_t)5 * R, *idxD = h + (size_t)6 * R;
  const int nA = p.nA, nC = p.nC, nD = p.nD;
  const int ld = e->max_L + 2;
  for (int q = 0; q < R; q++) memcpy(p.sorted.data() + off[q], seqs + p.src_off[p.order[q]], (size_t)h[q]);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_seqs, p.sorted.data(), p.total, hipMemcpyHostToDevice));
  reset_status(e);
  if ((want_pf || want_mfe) && nC) { const int rc = strip_flags(e, want_mfe); if (rc != DRNA_OK) return rc; }
  Ragged rg;
  rg.len = p.d_rg; rg.off = p.d_rg + R;
  HIP_TRY(hipEventRecord(e->ev_start, e->s_mfe));
  HIP_TRY(hipStreamWaitEvent(e->s_pf, e->ev_start, 0));
  HIP_TRY(hipStreamWaitEvent(e->s_eval, e->ev_start, 0));
  if (want_mfe) {
    MfeArgs a = mfe_args(e, e->d_seqs, 0, ld, want_pk ? 3 : 0, e->d_Emfe, e->d_ss);
    a.rg = rg;
    HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
    ragged_fold(e, R, h, idxA, nA, idxC, nC, idxD, nD, p.d_rg,
                [&](int c0) { a.ws = e->d_ws_mfe - (long long)c0 * a.ws_stride; a.rg.idx = nullptr; },
                [&](int n, int S, int k, const int* idx) { launch_mfe_strips(e, a, n, S, k, idx, e->s_mfe); },
                [&](int n, const int* idx) { a.rg.idx = idx; hipLaunchKernelGGL(mfe_kernel<1024>, dim3(n), dim3(1024), 0, e->s_mfe, a); },
                [&](int n, const int* idx) { a.rg.idx = idx; hipLaunchKernelGGL(mfe_lds_kernel<1024>, dim3(n), dim3(1024), 0, e->s_mfe, a); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
  }
  if (want_pf) {
    PfArgs a = pf_args(e, e->d_seqs, 0, ld, e->d_Epf);
    a.rg = rg;
    HIP_TRY(hipEventRecord(e->ev_p0, e->s_pf));
    ragged_fold(e, R, h, idxA, nA, idxC, nC, idxD, nD, p.d_rg,
                [&](int c0) { a.ws = e->d_ws_pf - (long long)c0 * a.ws_stride; a.rg.idx = nullptr; },
                [&](int n, int S, int k, const int* idx) { launch_pf_strips(e, a, n, S, k, idx, e->s_pf); },
                [&](int n, const int* idx) { a.rg.idx = idx; hipLaunchKernelGGL(pf_kernel<1024>, dim3(n), dim3(1024), 0, e->s_pf, a); },
                [&](int n, const int* idx) { a.rg.idx = idx; hipLaunchKernelGGL(pf_lds_kernel<1024>, dim3(n), dim3(1024), 0, e->s_pf, a, EvalArgs{}, n); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_p1, e->s_pf));
    HIP_TRY(hipStreamWaitEvent(e->s_mfe, e->ev_p1, 0));
  }
  if (want_ev) {
    EvalArgs a = eval_args(e, e->d_seqs, 0, e->d_Ed);
    a.pt = e->d_rpt; a.n_targets = 1;
    a.rg = rg; a.target_of = p.d_rg + (size_t)2 * R; a.pt_off = e->d_rpt_off;
    HIP_TRY(hipEventRecord(e->ev_e0, e->s_eval));
    hipLaunchKernelGGL(eval_kernel, dim3(R), dim3(WAVE), 0, e->s_eval, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_e1, e->s_eval));
    HIP_TRY(hipStreamWaitEvent(e->s_mfe, e->ev_e1, 0));
  }
  HIP_TRY(hipEventRecord(e->ev_end, e->s_mfe));
  HIP_TRY(hipStreamSynchronize(e->s_mfe));
  e->timing[0] = e->timing[1] = e->timing[2] = 0.f;
  if (want_mfe) HIP_TRY(hipEventElapsedTime(&e->timing[0], e->ev_m0, e->ev_m1));
  if (want_pf) HIP_TRY(hipEventElapsedTime(&e->timing[1], e->ev_p0, e->ev_p1));
  if (want_ev) HIP_TRY(hipEventElapsedTime(&e->timing[2], e->ev_e0, e->ev_e1));
  HIP_TRY(hipEventElapsedTime(&e->timing[3], e->ev_start, e->ev_end));
  bool lost = false;
  const int rc = fold_status(e, R, want_mfe, want_pf, p.order.data(), 0, "traceback could not reproduce a table value", &lost);
  if (lost && !e->in_fallback) return redo_solo(e, again);      // (see score_batch_impl)
  if (rc != DRNA_OK) return rc;
  if (!e->in_fallback) e->fallback_streak = 0;
  // results back in the caller's order
  if (want_pf) { const int rc = scatter_back(e, e->d_Epf, p.order, Epf); if (rc != DRNA_OK) return rc; }
  if (want_mfe) {
    { const int rc = scatter_back(e, e->d_Emfe, p.order, Emfe); if (rc != DRNA_OK) return rc; }
    HIP_TRY(hipMemcpy(p.sorted.data(), e->d_ss, p.total, hipMemcpyDeviceToHost));
    for (int q = 0; q < R; q++) memcpy(mfe_ss + p.src_off[p.order[q]], p.sorted.data() + off[q], (size_t)h[q]);
  }
  if (want_ev) { const int rc = scatter_back(e, e->d_Ed, p.order, Ed); if (rc != DRNA_OK) return rc; }
  return DRNA_OK;
}

extern "C" int drna_score_ragged(drna_engine* e, int R, const int32_t* lens, const char* seqs, const int32_t* target_of,
                                 uint32_t flags, double* Epf, int32_t* Emfe, char* mfe_ss, int32_t* Ed) {
  if (!e) return DRNA_ERR_ARG;
  const bool want_pf = flags & DRNA_NEED_PF, want_mfe = flags & (DRNA_NEED_MFE | DRNA_NEED_PK), want_ev = flags & DRNA_NEED_EVAL;
  if (R < 1 || R > e->max_R || !lens || !seqs || (want_pf && !Epf) || (want_mfe && (!Emfe || !mfe_ss)) ||
      (want_ev && (!Ed || !target_of))) {
    e->err = "drna_score_ragged: bad argument (R within the engine's limit; output pointers for every requested flag)";
    return DRNA_ERR_ARG;
  }
  RaggedPlan p;
  const int rc = ragged_plan(e, R, lens, target_of, flags, p);
  return rc != DRNA_OK ? rc : ragged_run(e, p, seqs, Epf, Emfe, mfe_ss, Ed);
}

// ---------------------------------------------------------------- ensemble defect of a ragged batch

// The plan of drna_ensemble_defect_ragged (made once per drna_mc_run_ragged_nd call): the layout of a ragged batch, split by the
// rule of the uniform path (edef_batch_device) per length -- with option "edef_lds" the sequences of at most EDEF_LDS_HOST_MAX
// nucleotides take the fused LDS kernel (list A), every other one pf_kernel + outside_kernel (list D, a prefix of the sorted order)
static int edef_ragged_plan(drna_engine* e, const char* who, int R, const int32_t* lens, const int32_t* target_of, RaggedPlan& p) {
  { const int rc = ragged_layout(e, who, R, lens, target_of, DRNA_NEED_EVAL, p); if (rc != DRNA_OK) return rc; }
  int *idxA = p.h.data() + (size_t)3 * R, *idxD = p.h.data() + (size_t)6 * R;
  p.nA = p.nC = p.nD = 0;
  for (int q = 0; q < R; q++) {
    if (e->edef_lds && p.h[q] <= EDEF_LDS_HOST_MAX) idxA[p.nA++] = q;
    else idxD[p.nD++] = q;
  }
  { const int rc = rg_block(e, RG_EDEF, &p.d_rg); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipMemcpy(p.d_rg, p.h.data(), p.h.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!e->d_edef) HIP_TRY(hipMalloc((void**)&e->d_edef, (size_t)e->max_R * sizeof(double)));
  if (!e->d_F4) HIP_TRY(hipMalloc((void**)&e->d_F4, (size_t)4 * e->max_R * sizeof(double)));
  return p.nD ? outside_workspace(e) : DRNA_OK;
}
// One pass of the plan's batch (seqs: the letters in the caller's order): list D in chunks of ws_slots positions, each chunk's
// two launches through inside_outside on the chunk's slots; then ONE launch of the fused kernel for all of list A, whatever their
// lengths.  A failed sequence is named by the caller's index; timing_edef = the sums over the chunks and the fused launch
static int edef_ragged_run(drna_engine* e, RaggedPlan& p, const char* seqs, double* edef) {
  const int R = p.R, ld = e->max_L + 2;
  const int *h = p.h.data(), *off = h + R;
  for (int q = 0; q < R; q++) memcpy(p.sorted.data() + off[q], seqs + p.src_off[p.order[q]], (size_t)h[q]);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_seqs, p.sorted.data(), p.total, hipMemcpyHostToDevice));
  Ragged rg;
  rg.len = p.d_rg; rg.off = p.d_rg + R;
  const int* d_target_of = p.d_rg + (size_t)2 * R;
  float sum[2] = {0, 0};
  int rc = DRNA_OK;
  if (p.nD) {
    PfArgs a = pf_args(e, e->d_seqs, 0, ld, e->d_Epf);
    a.rg = rg;
    a.q5_stride = outside_ws_stride(ld);
    OutArgs o;
    o.T = e->d_pfT; o.plan = e->d_plan; o.scale = e->d_scale; o.eMLb = e->d_eMLb;
    o.seqs = e->d_seqs; o.L = 0; o.ld = ld;
    o.ws_stride = a.ws_stride; o.wo_stride = a.q5_stride;
    o.pt = e->d_rpt; o.edef = e->d_edef; o.pf_status = e->d_status + e->max_R;
    o.rg = rg; o.target_of = d_target_of; o.pt_off = e->d_rpt_off;
    int c1 = 0;
    ragged_fold(e, R, h, nullptr, 0, nullptr, 0, h + (size_t)6 * R, p.nD, p.d_rg,
                [&](int c0) {            // the chunk's slots: every workspace pointer moved back by c0 slots
                  c1 = std::min(R, c0 + e->ws_slots);
                  a.ws = e->d_ws_pf - (long long)c0 * a.ws_stride;
                  o.wo = e->d_ws_out - (long long)c0 * o.wo_stride;
                  a.q5out = o.wo + (size_t)4 * ld * ld;
                  o.ws = a.ws;
                },
                [](int, int, int, const int*) {},
                [&](int n, const int* idx) {
                  if (rc != DRNA_OK) return;
                  a.rg.idx = o.rg.idx = idx;
                  rc = inside_outside(e, c1, 0, "unexpected status of the partition function",
                                      [&] { hipLaunchKernelGGL(pf_kernel<1024>, dim3(n), dim3(1024), 0, e->s_pf, a); },
                                      [&] { hipLaunchKernelGGL((outside_kernel<1024, true>), dim3(n), dim3(1024), 0, e->s_pf, o); },
                                      p.order.data());
                  sum[0] += e->timing_edef[0]; sum[1] += e->timing_edef[1];
                },
                [](int, const int*) {});
    if (rc != DRNA_OK) return rc;
  }
  if (p.nA) {
    EdefLdsArgs a;
    a.in = co_args(e, e->d_seqs, 0, 0, 0);
    a.out.F = e->d_pfT; a.out.plan = e->d_plan; a.out.scale = e->d_scale; a.out.eMLb = e->d_eMLb;
    a.out.seqs = e->d_seqs; a.out.eDuplexInit = a.in.eDuplexInit;
    a.out.pt = e->d_rpt; a.out.edef = e->d_edef; a.out.status_pf = a.in.status_pf;
    a.rg = rg; a.rg.idx = p.d_rg + (size_t)3 * R;
    a.target_of = d_target_of; a.pt_off = e->d_rpt_off;
    e->edef_lds_calls++;
    rc = inside_outside(e, R, 0, "unexpected status of the ensemble-defect kernel",
                        [&] { hipLaunchKernelGGL((edef_lds_kernel<1024, true, true>), dim3(p.nA), dim3(1024), 0, e->s_pf, a); }, [] {},
                        p.order.data());
    if (rc != DRNA_OK) return rc;
    sum[0] += e->timing_edef[0]; sum[1] += e->timing_edef[1];
  }
  e->timing_edef[0] = sum[0]; e->timing_edef[1] = sum[1];
  return scatter_back(e, e->d_edef, p.order, edef);
}

extern "C" int drna_ensemble_defect_ragged(drna_engine* e, int R, const int32_t* lens, const char* seqs, const int32_t* target_of,
                                           double* edef) {
  if (!e) return DRNA_ERR_ARG;
  const char* who = "drna_ensemble_defect_ragged";
  if (R < 1 || R > e->max_R || !lens || !seqs || !target_of || !edef) {
    e->err = std::string(who) + ": bad argument (R within the engine's limit max_R; lens, seqs, target_of and edef required)";
    return DRNA_ERR_ARG;
  }
  RaggedPlan p;
  const int rc = edef_ragged_plan(e, who, R, lens, target_of, p);
  return rc != DRNA_OK ? rc : edef_ragged_run(e, p, seqs, edef);
}

// ---------------------------------------------------------------- second-best structure energy (-nd on), one and two strands

// arguments of the three kernels of fold_subopt.hpp.  K = 2, the second-best folds: the tables live in the partition function's
// workspace, E2 comes back in d_Emfe, E12 in d_Epf.  K = 4 / 8, the ranked structures: everything in the K-best buffers.
static SuboptArgs subopt_args(const drna_engine* e, int L, int cut, int K) {
  SuboptArgs a;
  a.T = e->d_mfeT; a.plan = e->d_plan; a.hp_len = e->d_hp_len; a.seqs = e->d_seqs; a.L = L; a.cut = cut; a.ld = L + 2;
  a.DuplexInit = e->H.DuplexInit; a.status = e->d_status;
  if (K == 2) {
    a.ws = reinterpret_cast<int32_t*>(e->d_ws_pf); a.ws_stride = 2 * (long long)pf_ws_stride(L + 2);   // int32 units of the PF workspace
    a.E2 = e->d_Emfe; a.E12 = reinterpret_cast<int32_t*>(e->d_Epf);
  } else {
    a.ws = e->d_ws_kb; a.ws_stride = (long long)3 * K * a.ld * a.ld;
    a.E = e->d_kbE; a.ss = e->d_kbss;
  }
  return a;
}
// the second-best fold of R sequences (a.cut > 0: pairs) on the MFE stream: sequences of at most SUB_LDS_MAX nucleotides keep their
// tables in LDS (option "subopt_lds"), longer ones in the workspace slots
static void launch_second_best(drna_engine* e, const SuboptArgs& a, int R) {
  const bool lds = e->subopt_lds && a.L <= SUB_LDS_MAX;
  if (a.cut) {
    if (lds) hipLaunchKernelGGL(cofold_subopt_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
    else hipLaunchKernelGGL(cofold_subopt_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
  } else {
    if (lds) hipLaunchKernelGGL(subopt_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
    else hipLaunchKernelGGL(subopt_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
  }
}
// upload, launch() on the MFE stream (timed as "mfe"), status, E2 and (optional) E12 back
template <class Launch>
static int second_best_batch(drna_engine* e, int R, int L, const char* seqs, int32_t* E2, int32_t* E12, const char* internal_msg,
                             Launch&& launch) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_seqs, seqs, (size_t)R * L, hipMemcpyHostToDevice));
  reset_status(e);
  HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
  launch();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
  HIP_TRY(hipStreamSynchronize(e->s_mfe));
  HIP_TRY(hipEventElapsedTime(&e->timing[0], e->ev_m0, e->ev_m1));
  e->timing[1] = e->timing[2] = 0.f; e->timing[3] = e->timing[0];
  { const int rc = fold_status(e, R, true, false, nullptr, 0, internal_msg); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipMemcpy(E2, e->d_Emfe, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (E12) HIP_TRY(hipMemcpy(E12, e->d_Epf, (size_t)2 * R * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DRNA_OK;
}
static int second_best_check(drna_engine* e, const char* who, int R, int L, const int* cut, bool ok) {
  const int rc = aux_check(e, who, R, L, cut, ok, "seqs and E2 required");
  return rc != DRNA_OK ? rc : fits_workspace(e, who, R);
}

extern "C" int drna_subopt_energy_batch(drna_engine* e, int R, int L, const char* seqs, int32_t* E2, int32_t* E12) {
  if (!e) return DRNA_ERR_ARG;
  { const int rc = second_best_check(e, "drna_subopt_energy_batch", R, L, nullptr, seqs && E2); if (rc != DRNA_OK) return rc; }
  const SuboptArgs a = subopt_args(e, L, 0, 2);
  return second_best_batch(e, R, L, seqs, E2, E12, "unexpected status of the second-best fold",
                           [&] { launch_second_best(e, a, R); });
}

extern "C" int drna_cofold_subopt_energy_batch(drna_engine* e, int R, int L, int cut, const char* seqs, int32_t* E2, int32_t* E12) {
  if (!e) return DRNA_ERR_ARG;
  { const int rc = second_best_check(e, "drna_cofold_subopt_energy_batch", R, L, &cut, seqs && E2); if (rc != DRNA_OK) return rc; }
  const SuboptArgs a = subopt_args(e, L, cut, 2);
  return second_best_batch(e, R, L, seqs, E2, E12, "unexpected status of the second-best co-fold",
                           [&] { launch_second_best(e, a, R); });
}

// The negative-design step of the native loops: H sequences (L letters each; cut > 0: pairs without the '&') the caller has put
// into hm_seqs; E2 comes back in hm_Emfe, so the step costs one launch and no hipMemcpy
static int second_best_mapped(drna_engine* e, int H, int L, int cut) {
  HIP_TRY(hipSetDevice(e->device));
  reset_status(e);
  SuboptArgs a = subopt_args(e, L, cut, 2);
  a.seqs = e->dm_seqs; a.E2 = e->dm_Emfe; a.E12 = nullptr;
  launch_second_best(e, a, H);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->s_mfe));
  return fold_status(e, H, true, false, nullptr, 0, cut ? "unexpected status of the second-best co-fold" : "unexpected status of the second-best fold");
}

// The second-best folds of R sequences of lengths lens (one strand), their letters one after the other at d_seqs (device or
// host-mapped), in one launch per kernel: with option "subopt_lds" the sequences of at most SUB_LDS_MAX nucleotides keep their
// tables in LDS, the others use their workspace slot.  Nothing is permuted: the descriptors len | off are in the caller's order
// and a workgroup list (longest first; the general kernel's part is its prefix) maps workgroups to sequences, so E2 / E12, the
// status word and the workspace slot of sequence r are at r (R <= ws_slots, fits_workspace) and an error names the caller's index
static int second_best_ragged(drna_engine* e, int R, const int32_t* lens, const char* d_seqs, int32_t* d_E2,
                              int32_t* d_E12) {
  std::vector<int> h((size_t)3 * R), order(R);
  longest_first(order, lens);
  int nG = 0;
  { int o = 0; for (int r = 0; r < R; r++) { h[r] = lens[r]; h[(size_t)R + r] = o; o += lens[r]; } }
  for (int q = 0; q < R; q++) {
    h[(size_t)2 * R + q] = order[q];
    nG += !(e->subopt_lds && lens[order[q]] <= SUB_LDS_MAX);
  }
  int* d_rg = nullptr;
  { const int rc = rg_block(e, RG_SUB, &d_rg); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipMemcpy(d_rg, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  reset_status(e);
  SuboptArgs a = subopt_args(e, e->max_L, 0, 2);       // slots of the largest size; the kernels take length and pitch from rg
  a.L = 0;
  a.seqs = d_seqs; a.E2 = d_E2; a.E12 = d_E12;
  a.rg.len = d_rg; a.rg.off = d_rg + R;
  HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
  if (nG) { a.rg.idx = d_rg + (size_t)2 * R; hipLaunchKernelGGL((subopt_kernel<1024, true>), dim3(nG), dim3(1024), 0, e->s_mfe, a); }
  if (R - nG) { a.rg.idx = d_rg + (size_t)2 * R + nG; hipLaunchKernelGGL((subopt_lds_kernel<1024, true>), dim3(R - nG), dim3(1024), 0, e->s_mfe, a); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
  HIP_TRY(hipStreamSynchronize(e->s_mfe));
  HIP_TRY(hipEventElapsedTime(&e->timing[0], e->ev_m0, e->ev_m1));
  e->timing[1] = e->timing[2] = 0.f; e->timing[3] = e->timing[0];
  return fold_status(e, R, true, false, nullptr, 0, "unexpected status of the second-best fold");
}

extern "C" int drna_subopt_energy_ragged(drna_engine* e, int R, const int32_t* lens, const char* seqs, int32_t* E2, int32_t* E12) {
  if (!e) return DRNA_ERR_ARG;
  const char* who = "drna_subopt_energy_ragged";
  if (R < 1 || R > e->max_R || !lens || !seqs || !E2) {
    e->err = std::string(who) + ": bad argument (R within the engine's limit max_R; lens, seqs and E2 required)";
    return DRNA_ERR_ARG;
  }
  { const int rc = fits_workspace(e, who, R); if (rc != DRNA_OK) return rc; }
  size_t total = 0;
  for (int r = 0; r < R; r++) {
    if (lens[r] < 1 || lens[r] > e->max_L) {
      e->err = std::string(who) + ": sequence " + std::to_string(r) + ": length outside [1, max_L]";
      return DRNA_ERR_ARG;
    }
    total += (size_t)lens[r];
  }
  if (total > (size_t)e->max_R * e->max_L) { e->err = std::string(who) + ": more nucleotides than max_R * max_L"; return DRNA_ERR_ARG; }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_seqs, seqs, total, hipMemcpyHostToDevice));
  { const int rc = second_best_ragged(e, R, lens, e->d_seqs, e->d_Emfe, E12 ? reinterpret_cast<int32_t*>(e->d_Epf) : nullptr); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipMemcpy(E2, e->d_Emfe, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (E12) HIP_TRY(hipMemcpy(E12, e->d_Epf, (size_t)2 * R * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DRNA_OK;
}

// the ranked structures of R sequences (cut > 0: pairs) through the K-best workspace in chunks of kb_chunk.  One slot size serves
// both kernels (the two-strand one keeps its 1-D lists and stacks behind the three tables), whichever call comes first
static int ranked_structs_batch(drna_engine* e, int R, int L, int cut, const char* seqs, int K, int32_t* E, char* ss) {
  HIP_TRY(hipSetDevice(e->device));
  const int KT = K <= 4 ? 4 : 8;                      // kernel instantiations
  const int ldmax = e->max_L + 2;
  const size_t stride_max = (size_t)3 * 8 * ldmax * ldmax + (size_t)cofold_kbest_ws_extra(8, ldmax);
  if (!e->d_ws_kb) {
    e->kb_chunk = e->max_R < 16 ? e->max_R : 16;
    HIP_TRY(hipMalloc((void**)&e->d_ws_kb, stride_max * sizeof(int32_t) * e->kb_chunk));
    HIP_TRY(hipMalloc((void**)&e->d_kbE, (size_t)8 * e->kb_chunk * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&e->d_kbss, (size_t)8 * e->kb_chunk * e->max_L));
    e->ws_bytes += stride_max * sizeof(int32_t) * e->kb_chunk;
  }
  std::vector<int32_t> hE((size_t)KT * e->kb_chunk);
  std::vector<char> hs((size_t)KT * e->kb_chunk * L);
  float ms_total = 0.f;
  for (int r0 = 0; r0 < R; r0 += e->kb_chunk) {
    const int rc = R - r0 < e->kb_chunk ? R - r0 : e->kb_chunk;
    HIP_TRY(hipMemcpy(e->d_seqs, seqs + (size_t)r0 * L, (size_t)rc * L, hipMemcpyHostToDevice));
    for (int k = 0; k < rc; k++) e->h_status[k] = ST_OK;
    SuboptArgs a = subopt_args(e, L, cut, KT);
    if (cut) a.ws_stride += cofold_kbest_ws_extra(KT, a.ld);
    HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
    if (cut) {
      if (KT == 4) hipLaunchKernelGGL((cofold_kbest_kernel<1024, 4>), dim3(rc), dim3(1024), 0, e->s_mfe, a);
      else hipLaunchKernelGGL((cofold_kbest_kernel<1024, 8>), dim3(rc), dim3(1024), 0, e->s_mfe, a);
    } else {
      if (KT == 4) hipLaunchKernelGGL((kbest_kernel<1024, 4>), dim3(rc), dim3(1024), 0, e->s_mfe, a);
      else hipLaunchKernelGGL((kbest_kernel<1024, 8>), dim3(rc), dim3(1024), 0, e->s_mfe, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
    HIP_TRY(hipStreamSynchronize(e->s_mfe));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev_m0, e->ev_m1));
    ms_total += ms;
    { const int st = fold_status(e, rc, true, false, nullptr, r0, "traceback of a ranked structure failed (internal error)"); if (st != DRNA_OK) return st; }
    HIP_TRY(hipMemcpy(hE.data(), e->d_kbE, (size_t)KT * rc * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hs.data(), e->d_kbss, (size_t)KT * rc * L, hipMemcpyDeviceToHost));
    for (int r = 0; r < rc; r++)
      for (int k = 0; k < K; k++) {
        E[(size_t)(r0 + r) * K + k] = hE[(size_t)r * KT + k];
        memcpy(ss + ((size_t)(r0 + r) * K + k) * L, hs.data() + ((size_t)r * KT + k) * L, (size_t)L);
      }
  }
  e->timing[0] = ms_total; e->timing[1] = e->timing[2] = 0.f; e->timing[3] = ms_total;
  return DRNA_OK;
}

extern "C" int drna_subopt_structs_batch(drna_engine* e, int R, int L, const char* seqs, int K, int32_t* E, char* ss) {
  if (!e) return DRNA_ERR_ARG;
  // (no upper limit on R here: the batch goes through the K-best workspace in chunks of kb_chunk)
  { const int rc = aux_check(e, "drna_subopt_structs_batch", std::min(R, e->max_R), L, nullptr, K >= 1 && K <= 8 && seqs && E && ss,
                             "1 <= K <= 8; seqs, E and ss required"); if (rc != DRNA_OK) return rc; }
  return ranked_structs_batch(e, R, L, 0, seqs, K, E, ss);
}

extern "C" int drna_cofold_subopt_structs_batch(drna_engine* e, int R, int L, int cut, const char* seqs, int K, int32_t* E, char* ss) {
  if (!e) return DRNA_ERR_ARG;
  { const int rc = aux_check(e, "drna_cofold_subopt_structs_batch", std::min(R, e->max_R), L, &cut, K >= 1 && K <= 8 && seqs && E && ss,
                             "1 <= K <= 8; seqs, E and ss required"); if (rc != DRNA_OK) return rc; }
  return ranked_structs_batch(e, R, L, cut, seqs, K, E, ss);
}

// ---------------------------------------------------------------- two strands (co-fold)

// R pairs whose letters the caller has put into hm_seqs (L each, no '&'): both folds side by side on their streams and the
// two-strand evaluation, every result written by the kernels into the host-mapped buffers (hm_F4, hm_Emfe, hm_ss, hm_Ed), so a
// batch costs no hipMemcpy.  Pairs of at most CO_LDS_MAX nucleotides take the LDS-resident kernels (option "cofold_lds")
static int mapped_F4(drna_engine* e) {
  if (e->hm_F4) return DRNA_OK;
  HIP_TRY(hipHostMalloc((void**)&e->hm_F4, (size_t)4 * e->max_R * sizeof(double), hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void**)&e->dm_F4, e->hm_F4, 0));
  return DRNA_OK;
}
static int cofold_batch_mapped(drna_engine* e, int R, int L, int cut, bool want_pf, bool want_mfe, bool want_ev) {
  HIP_TRY(hipSetDevice(e->device));
  { const int rc = mapped_F4(e); if (rc != DRNA_OK) return rc; }
  if (want_ev) { const int rc = mapped_Ed(e); if (rc != DRNA_OK) return rc; }
  reset_status(e);
  CoArgs a = co_args(e, e->dm_seqs, L, cut, L + 2);
  a.F4 = e->dm_F4; a.Emfe = e->dm_Emfe; a.ss = e->dm_ss;
  const bool lds = e->cofold_lds && L <= CO_LDS_MAX;
  HIP_TRY(hipEventRecord(e->ev_p0, e->s_pf));
  HIP_TRY(hipEventRecord(e->ev_m0, e->s_mfe));
  if (want_pf) {
    if (lds) hipLaunchKernelGGL(cofold_pf_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, a);
    else hipLaunchKernelGGL(cofold_pf_kernel<1024>, dim3(R), dim3(1024), 0, e->s_pf, a);
  }
  if (want_mfe) {
    if (lds) hipLaunchKernelGGL(cofold_mfe_lds_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
    else hipLaunchKernelGGL(cofold_mfe_kernel<1024>, dim3(R), dim3(1024), 0, e->s_mfe, a);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_p1, e->s_pf));
  HIP_TRY(hipEventRecord(e->ev_m1, e->s_mfe));
  if (want_ev) {
    EvalArgs v = eval_args(e, e->dm_seqs, L, e->dm_Ed);
    v.cut = cut; v.DuplexInit = e->H.DuplexInit;
    hipLaunchKernelGGL(eval_kernel, dim3(R * e->n_targets), dim3(WAVE), 0, e->s_eval, v);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(e->s_pf));
  HIP_TRY(hipStreamSynchronize(e->s_mfe));
  HIP_TRY(hipStreamSynchronize(e->s_eval));
  HIP_TRY(hipEventElapsedTime(&e->timing[0], e->ev_m0, e->ev_m1));
  HIP_TRY(hipEventElapsedTime(&e->timing[1], e->ev_p0, e->ev_p1));
  e->timing[2] = 0.f; e->timing[3] = e->timing[0] > e->timing[1] ? e->timing[0] : e->timing[1];
  return fold_status(e, R, want_mfe, want_pf, nullptr, 0, "traceback could not reproduce a table value");
}

extern "C" int drna_cofold_batch(drna_engine* e, int R, int L, int cut, const char* seqs, uint32_t flags, double* F4,
                                 int32_t* Emfe, char* mfe_ss, int32_t* Ed) {
  if (!e) return DRNA_ERR_ARG;
  const bool want_pf = flags & DRNA_NEED_PF, want_mfe = flags & DRNA_NEED_MFE, want_ev = flags & DRNA_NEED_EVAL;
  const char* who = "drna_cofold_batch";
  int rc = aux_check(e, who, R, L, &cut, seqs && (!want_pf || F4) && (!want_mfe || (Emfe && mfe_ss)) && (!want_ev || Ed) && !(flags & DRNA_NEED_PK),
                     "output pointers for every requested flag; no NEED_PK");
  if (rc == DRNA_OK && want_ev) rc = need_targets(e, who, L);
  if (rc == DRNA_OK) rc = fits_workspace(e, who, R);
  if (rc != DRNA_OK) return rc;
  std::memcpy(e->hm_seqs, seqs, (size_t)R * L);
  rc = cofold_batch_mapped(e, R, L, cut, want_pf, want_mfe, want_ev);
  if (rc != DRNA_OK) return rc;
  if (want_pf) std::memcpy(F4, e->hm_F4, (size_t)4 * R * sizeof(double));
  if (want_mfe) {
    std::memcpy(Emfe, e->hm_Emfe, (size_t)R * sizeof(int32_t));
    std::memcpy(mfe_ss, e->hm_ss, (size_t)R * L);
  }
  if (want_ev) std::memcpy(Ed, e->hm_Ed, (size_t)R * e->n_targets * sizeof(int32_t));
  return DRNA_OK;
}

// ---------------------------------------------------------------- a sequence against a copy of itself (-oa on)

// reference utils/dimer_multichain_energy.py:24-45: fraction of strands bound in the dimer at 1 mM, and -kT ln of a fraction
static double oligo_fraction(double FA, double FB, double FcAB) {
  const double KB = 0.001987204259, RHO = 55.14, TEMP = 273.15 + 37, CONC = 1e-3;
  const double dF = FcAB - FA - FB;
  const double rhs = CONC / RHO * std::exp(-dF / (KB * TEMP));
  return 1 - (std::sqrt(1 + 4 * rhs) - 1) / (2 * rhs);
}
static double kT_log(double x) { return -0.001987204259 * (273.15 + 37) * std::log(x); }

// H sequences (L letters each) the caller has put into hm_seqs: the partition function of each against a copy of itself in ONE
// launch on the partition function's stream, F4 into hm_F4 (no hipMemcpy).  The caller's other launches have drained: the kernel
// is never resident beside the fused / two-workgroup folds, which size their grids against the whole chip.  Sequences of at most
// SD_LDS_MAX nucleotides keep their tables in LDS (option "self_dimer_lds"); longer ones use the partition function's workspace
// slots, which hold more than the ~1.5 L^2 cells of the three tables (4.7 L^2 against 7.1 (L + 2)^2 doubles)
static int self_dimer_mapped(drna_engine* e, int H, int L) {
  HIP_TRY(hipSetDevice(e->device));
  { const int rc = mapped_F4(e); if (rc != DRNA_OK) return rc; }
  if (sd_ws_stride(L) > (long long)pf_ws_stride(e->max_L + 2)) { e->err = "self-dimer: workspace slot too small"; return DRNA_ERR_INTERNAL; }
  reset_status(e);
  CoArgs a = co_args(e, e->dm_seqs, L, L, L + 2);
  a.wsp_stride = (long long)pf_ws_stride(e->max_L + 2);
  a.F4 = e->dm_F4;
  HIP_TRY(hipEventRecord(e->ev_p0, e->s_pf));
  if (e->self_dimer_lds && L <= SD_LDS_MAX) hipLaunchKernelGGL(self_dimer_pf_lds_kernel<1024>, dim3(H), dim3(1024), 0, e->s_pf, a);
  else hipLaunchKernelGGL(self_dimer_pf_kernel<1024>, dim3(H), dim3(1024), 0, e->s_pf, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_p1, e->s_pf));
  HIP_TRY(hipStreamSynchronize(e->s_pf));
  HIP_TRY(hipEventElapsedTime(&e->timing[1], e->ev_p0, e->ev_p1));
  e->timing[0] = e->timing[2] = 0.f; e->timing[3] = e->timing[1];
  return fold_status(e, H, false, true, nullptr, 0, "unexpected status of the self-dimer partition function");
}

extern "C" int drna_self_dimer_batch(drna_engine* e, int R, int L, const char* seqs, double* F4, double* oligo_frac) {
  if (!e) return DRNA_ERR_ARG;
  // (no upper limit on R: the batch goes through the workspace slots in chunks)
  { const int rc = aux_check(e, "drna_self_dimer_batch", std::min(R, e->max_R), L, nullptr, seqs && F4, "seqs and F4 required"); if (rc != DRNA_OK) return rc; }
  float ms = 0.f;
  for (int r0 = 0; r0 < R; r0 += e->ws_slots) {
    const int m = std::min(R - r0, e->ws_slots);
    std::memcpy(e->hm_seqs, seqs + (size_t)r0 * L, (size_t)m * L);
    const int rc = self_dimer_mapped(e, m, L);
    if (rc != DRNA_OK) return rc;
    std::memcpy(F4 + (size_t)4 * r0, e->hm_F4, (size_t)4 * m * sizeof(double));
    ms += e->timing[1];
  }
  e->timing[1] = e->timing[3] = ms;
  if (oligo_frac)
    for (int r = 0; r < R; r++) oligo_frac[r] = oligo_fraction(F4[4 * (size_t)r], F4[4 * (size_t)r + 1], F4[4 * (size_t)r + 2]);
  return DRNA_OK;
}

// ---------------------------------------------------------------- partition function with positions held unpaired (fold_access.hpp)

// m (sequence, mask) pairs, g0 the first (pair g = sequence g / M under mask g % M), whose sequences -- seq0 the first -- the
// caller has put into hm_seqs and whose M masks are in d_nopair: ONE launch on the partition function's stream, pair g0 + b in
// workspace slot / status word b, F into hm_Epf[b] (general kernel) or hm_F4[4 b] (tables in LDS); no hipMemcpy.  The caller's
// other launches have drained (the self-dimer step's rule).  An error names the pair's sequence
static int access_mapped(drna_engine* e, int m, int L, int M, int g0, int seq0, bool lds) {
  reset_status(e);
  HIP_TRY(hipEventRecord(e->ev_p0, e->s_pf));
  if (lds) {
    AccessLdsArgs a;
    a.in = co_args(e, e->dm_seqs, L, L, 0);
    a.in.F4 = e->dm_F4;
    a.nopair = e->d_nopair; a.M = M; a.fold0 = g0; a.seq0 = seq0;
    e->access_lds_calls++;
    hipLaunchKernelGGL(access_lds_kernel<1024>, dim3(m), dim3(1024), 0, e->s_pf, a);
  } else {
    PfMaskArgs a;
    static_cast<PfArgs&>(a) = pf_args(e, e->dm_seqs, L, L + 2, e->dm_Epf);
    a.nopair = e->d_nopair; a.M = M; a.fold0 = g0; a.seq0 = seq0;
    hipLaunchKernelGGL((pf_kernel<1024, true>), dim3(m), dim3(1024), 0, e->s_pf, a);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e->ev_p1, e->s_pf));
  HIP_TRY(hipStreamSynchronize(e->s_pf));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e->ev_p0, e->ev_p1));
  e->timing_access += ms;
  std::vector<int> order(m);
  for (int b = 0; b < m; b++) order[b] = (g0 + b) / M;
  return fold_status(e, m, false, true, order.data(), 0, "unexpected status of the masked partition function");
}

extern "C" int drna_pf_unpaired_batch(drna_engine* e, int R, int L, const char* seqs, int M, const unsigned char* nopair, double* F) {
  if (!e) return DRNA_ERR_ARG;
  // (no upper limit on R or M: the R M folds go through the workspace slots in chunks)
  { const int rc = aux_check(e, "drna_pf_unpaired_batch", std::min(R, e->max_R), L, nullptr, M >= 1 && (long long)R * M <= 0x7fffffffll && seqs && nopair && F,
                             "M >= 1, R M < 2^31; seqs, nopair and F required"); if (rc != DRNA_OK) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  const bool lds = e->access_lds && L <= (e->access_lds_force ? ACCESS_LDS_MAX : ACCESS_LDS_HOST_MAX);
  if (lds) { const int rc = mapped_F4(e); if (rc != DRNA_OK) return rc; }
  const size_t mb = (size_t)M * L;
  if (mb > e->nopair_cap) {
    if (e->d_nopair) (void)hipFree(e->d_nopair);
    e->d_nopair = nullptr; e->nopair_cap = 0;
    HIP_TRY(hipMalloc((void**)&e->d_nopair, mb));
    e->nopair_cap = mb;
  }
  HIP_TRY(hipMemcpy(e->d_nopair, nopair, mb, hipMemcpyHostToDevice));
  e->timing_access = 0.f;
  // the LDS kernel needs no workspace slot: its chunks are bounded by the status words and the staging buffers alone
  const long long total = (long long)R * M, step = lds ? e->max_R : e->ws_slots;
  for (long long g0 = 0; g0 < total; g0 += step) {
    const int m = (int)std::min(step, total - g0);
    const int s0 = (int)(g0 / M), s1 = (int)((g0 + m - 1) / M);          // the chunk's sequences: at most m of them
    std::memcpy(e->hm_seqs, seqs + (size_t)s0 * L, (size_t)(s1 - s0 + 1) * L);
    const int rc = access_mapped(e, m, L, M, (int)g0, s0, lds);
    if (rc != DRNA_OK) return rc;
    for (int b = 0; b < m; b++) F[g0 + b] = lds ? e->hm_F4[4 * (size_t)b] : e->hm_Epf[b];
  }
  return DRNA_OK;
}

extern "C" int drna_last_access_timing(const drna_engine* e, float* ms) {
  if (!e || !ms) return DRNA_ERR_ARG;
  *ms = e->timing_access;
  return DRNA_OK;
}

// ---------------------------------------------------------------- host-side batched MC helpers (no device work)

extern "C" int drna_simscore_batch(int R, int L, const char* ref, const char* queries, double* mcc, double* recall,
                                   double* precision) {
  using namespace drna_host;
  if (R < 0 || L < 1 || L > 2048 || !ref || (R > 0 && (!queries || !mcc || !recall || !precision))) return DRNA_ERR_ARG;
  std::vector<int> pr(L), pq(L);
  if (!pair_table(ref, L, pr.data())) return DRNA_ERR_STRUCTURE;
  for (int r = 0; r < R; r++) {
    if (!pair_table(queries + (size_t)r * L, L, pq.data())) return DRNA_ERR_STRUCTURE;
    const SimMetrics m = sim_metrics(pr.data(), pq.data(), L);
    mcc[r] = m.mcc; recall[r] = m.recall; precision[r] = m.precision;
  }
  return DRNA_OK;
}

extern "C" int drna_motif_score_batch(int R, int L, const char* seqs, int n_motifs, const int32_t* motif_len, const char* motifs,
                                      const double* value, double* out) {
  using namespace drna_host;
  if (R < 0 || L < 1 || n_motifs < 0 || (R > 0 && (!seqs || !out)) || (n_motifs > 0 && (!motif_len || !motifs || !value))) return DRNA_ERR_ARG;
  MotifSet set;
  if (!motif_compile(n_motifs, motif_len, motifs, value, set)) return DRNA_ERR_ARG;
  for (int r = 0; r < R; r++) out[r] = motif_score(set, seqs + (size_t)r * L, L);
  return DRNA_OK;
}

extern "C" int drna_set_motifs(drna_engine* e, int n_motifs, const int32_t* motif_len, const char* motifs, const double* value) {
  if (!e) return DRNA_ERR_ARG;
  if (n_motifs < 0 || (n_motifs > 0 && (!motif_len || !motifs || !value))) { e->err = "drna_set_motifs: bad argument"; return DRNA_ERR_ARG; }
  if (!drna_host::motif_compile(n_motifs, motif_len, motifs, value, e->motifs)) {          // (the engine's set stays as it was)
    e->err = "drna_set_motifs: a motif holds a letter other than A C G T U W S M K R Y B D H V N, or has a negative length";
    return DRNA_ERR_ARG;
  }
  return DRNA_OK;
}

extern "C" int drna_rng_seed(int R, const uint64_t* seeds, uint32_t* rng_state) {
  if (R < 0 || (R > 0 && (!seeds || !rng_state))) return DRNA_ERR_ARG;
  for (int r = 0; r < R; r++) drna_host::mt_seed_int(drna_host::Mt{rng_state + (size_t)r * drna_host::RNG_WORDS}, seeds[r]);
  return DRNA_OK;
}

extern "C" int drna_rng_random(int R, uint32_t* rng_state, double* out) {
  if (R < 0 || (R > 0 && (!rng_state || !out))) return DRNA_ERR_ARG;
  for (int r = 0; r < R; r++) out[r] = drna_host::rnd01(drna_host::Mt{rng_state + (size_t)r * drna_host::RNG_WORDS});
  return DRNA_OK;
}

// The design problem as the proposer sees it, built once per call (drna_propose_batch*) or per exchange step (drna_mc_run):
// pair tables of the target and of all design pairs, the mutable positions, the snakes of alternative-structure designs
struct ProposeCtx {
  int L = 0, n_shelves = 1, targeted = 0;
  double tm_max = 0, tm_min = 0;
  const unsigned char* allowed_mask = nullptr;
  const int32_t *snake_of = nullptr, *snake_off = nullptr, *snake_nodes = nullptr, *snake_nstates = nullptr;
  const char* snake_states = nullptr;
  std::vector<int> pt, pd, mutable_pos;
  // two strands (drna_propose_batch_co, drna_mc_run_cofold): the strings keep the '&' at column amp (-1: one strand) as a fixed,
  // unpaired letter; homodimer: the reference's strand-copy rules follow every move, ss_equal = both sub-structures are the same
  int amp = -1;
  bool homodimer = false, ss_equal = false;
  bool fixed(int i) const { return i == amp || __builtin_popcount(allowed_mask[i] & 15u) == 1; }
};
// the two-strand part of a context built by propose_ctx_init: target and every string carry the '&' at the same column
static int propose_ctx_two_strands(ProposeCtx& c, const char* target, int oligo_state) {
  const int L = c.L;
  int amp = -1;
  for (int i = 0; i < L; i++)
    if (target[i] == '&') { if (amp >= 0) return DRNA_ERR_ARG; amp = i; }
  if (amp < 1 || amp > L - 2 || (oligo_state != 1 && oligo_state != 2)) return DRNA_ERR_ARG;
  c.amp = amp;
  c.homodimer = oligo_state == 2;
  c.ss_equal = L - amp - 1 == amp && std::memcmp(target, target + amp + 1, (size_t)amp) == 0;
  c.mutable_pos.clear();
  for (int i = 0; i < L; i++)
    if (!c.fixed(i)) c.mutable_pos.push_back(i);
  return c.mutable_pos.empty() ? DRNA_ERR_ARG : DRNA_OK;
}
static int propose_ctx_init(ProposeCtx& c, int L, const char* target, const int32_t* partner, const unsigned char* allowed_mask,
                            const int32_t* snake_of, const int32_t* snake_off, const int32_t* snake_nodes,
                            const int32_t* snake_nstates, const char* snake_states, int n_shelves, double tm_max, double tm_min,
                            int targeted) {
  using namespace drna_host;
  c.L = L; c.n_shelves = n_shelves; c.targeted = targeted; c.tm_max = tm_max; c.tm_min = tm_min; c.allowed_mask = allowed_mask;
  c.snake_of = snake_of; c.snake_off = snake_off; c.snake_nodes = snake_nodes; c.snake_nstates = snake_nstates; c.snake_states = snake_states;
  c.pt.assign(L, -1); c.pd.assign(L, -1); c.mutable_pos.clear();
  if (!pair_table(target, L, c.pt.data())) return DRNA_ERR_STRUCTURE;
  for (int i = 0; i < L; i++) {
    c.pd[i] = partner ? partner[i] : c.pt[i];
    if (c.pd[i] >= L || (c.pd[i] >= 0 && (partner ? partner[c.pd[i]] : c.pt[c.pd[i]]) != i)) return DRNA_ERR_ARG;
  }
  for (int i = 0; i < L; i++)
    if (__builtin_popcount(allowed_mask[i] & 15u) != 1) c.mutable_pos.push_back(i);
  if (c.mutable_pos.empty()) return DRNA_ERR_ARG;
  return DRNA_OK;
}
// round(numpy.linspace(tm_max, tm_min, n_shelves)[shelf], 2): linspace is start + k * step with the last point set to the stop
// value; round() is the correctly rounded decimal, like printf
static double shelf_probability(const ProposeCtx& c, int shelf) {
  double p = c.tm_max;
  if (c.n_shelves > 1) {
    const double step = (c.tm_min - c.tm_max) / (double)(c.n_shelves - 1);
    p = shelf == c.n_shelves - 1 ? c.tm_min : (double)shelf * step + c.tm_max;
  }
  char buf[32]; snprintf(buf, sizeof buf, "%.2f", p);
  return strtod(buf, nullptr);
}
// targeted moves: the positions a proposal may pick from = ends of false-negative / false-positive pairs of the current MFE
// structure (pair table pq) against the target, widened by +-3 (position 0 never enters); returns their number (0: none).
// mark is scratch of L entries.  The pool depends on the replica's CURRENT structure only, so drna_mc_run keeps it until a
// proposal is accepted
static int targeted_pool(const ProposeCtx& c, const int* pq, char* mark, int* pool) {
  const int L = c.L;
  std::memset(mark, 0, (size_t)L);
  bool any = false;
  for (int i = 0; i < L; i++)
    if (c.pt[i] != pq[i] && (c.pt[i] >= 0 || pq[i] >= 0) && !c.fixed(i)) {
      any = true;                                       // end of a false-negative or false-positive pair
      for (int k = -3; k <= 3; k++) { const int x = i + k; if (x > 0 && x <= L - 1) mark[x] = 1; }
    }
  int np = 0;
  if (any)
    for (int i = 0; i < L; i++) if (mark[i]) pool[np++] = i;
  return any ? np : -1;                                  // -1: no mispaired position (no draw is made then)
}
// Homodimer designs: the reference's strand-copy rules after a move at pos (utils/sequence_utils.py:1104-1126), s = the sequence
// before the move, o = after it.  Two different sub-structures: a pair move outside a snake is crossed over, strand 1 takes the
// letter of strand 2 at the pair's second end (as an index into strand 2) and strand 2 that of strand 1 at the first end.  Two
// equal sub-structures: the strand that changed is copied over the other.  The reference does the first with Python slices
// (s1[:b] + s2[b] + s1[b+1:]); an index that would change a string's length there (b = -1, an index past the end) is an error here
static int homodimer_copy(const ProposeCtx& c, const char* s, int pos, char* o) {
  const int len1 = c.amp, len2 = c.L - c.amp - 1;
  char *s1 = o, *s2 = o + len1 + 1;
  const int j = c.pd[pos];
  if (j >= 0 && !(c.snake_of && c.snake_of[pos] >= 0) && !c.ss_equal) {
    const int a = pos < j ? pos : j, b = (pos < j ? j : pos) - len1 - 1;
    // Python's index rules: a negative index counts from the end
    if (a >= len1 || a >= len2 || b >= len1 || b >= len2 || b == -1 || b < -len1 || b < -len2) return DRNA_ERR_ARG;
    const char from2 = s2[b >= 0 ? b : len2 + b], from1 = s1[a];
    s1[b >= 0 ? b : len1 + b] = from2;
    s2[a] = from1;
  }
  if (c.ss_equal) {
    if (std::memcmp(s1, s, (size_t)len1) != 0) std::memcpy(s2, s1, (size_t)len1);
    else if (std::memcmp(s2, s + len1 + 1, (size_t)len2) != 0) std::memcpy(s1, s2, (size_t)len1);
  }
  return DRNA_OK;
}

// one proposal of one replica: s = its sequence, pool / np = targeted_pool of its current MFE structure (np = -1 without targeted
// moves), p_shelf = shelf_probability of its temperature shelf
static int propose_one(const ProposeCtx& c, const char* s, const int* pool, int np, double p_shelf, drna_host::Mt st, char* o) {
  using namespace drna_host;
  static const char LET[4] = {'A', 'C', 'G', 'U'};
  static const unsigned CANPAIR[4] = {8u, 4u, 2u | 8u, 1u | 4u};   // A-U, C-G, G-C/U, U-A/G
  const int L = c.L;
  const unsigned char* allowed_mask = c.allowed_mask;
  auto letter_index = [](char ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3; };
  std::memcpy(o, s, (size_t)L);
  int pos = -1;
  if (np >= 0 && rnd_choices2(st, p_shelf) == 0 && np > 0)          // choices([expanded, mutable], weights=[p, 1 - p])
    pos = pool[rnd_below(st, np)];
  if (pos < 0) pos = c.mutable_pos[rnd_below(st, (int)c.mutable_pos.size())];
  const unsigned am = allowed_mask[pos] & 15u;
  const int cur = letter_index(s[pos]);
  const int j = c.pd[pos];
  if (c.snake_of && c.snake_of[pos] >= 0) {
    // alternative structures: the whole connected component moves to another of its Watson-Crick colourings
    // (reference utils/sequence_utils.py:1081-1095)
    const int k = c.snake_of[pos], n0 = c.snake_off[k], len = c.snake_off[k + 1] - n0, ns = c.snake_nstates[k];
    const char* states = c.snake_states + (size_t)4 * n0;
    int x = 0;
    while (x < len && c.snake_nodes[n0 + x] != pos) x++;
    if (x == len) return DRNA_ERR_ARG;
    int curst = -1;
    for (int q = 0; q < ns; q++) if (states[(size_t)q * len + x] == s[pos]) { curst = q; break; }
    const int nopt = ns - (curst >= 0 ? 1 : 0);
    if (nopt > 0) {
      int pick = rnd_below(st, nopt);
      if (curst >= 0 && pick >= curst) pick++;
      for (int y = 0; y < len; y++) o[c.snake_nodes[n0 + y]] = states[(size_t)pick * len + y];
    }
  } else if (j < 0) {
    unsigned opts = __builtin_popcount(am) > 1 ? (am & ~(1u << cur)) : 0u;
    if (opts) {
      int k = rnd_below(st, __builtin_popcount(opts));
      for (int b = 0; b < 4; b++) if (opts & (1u << b)) { if (!k--) { o[pos] = LET[b]; break; } }
    }
  } else {
    unsigned o1 = __builtin_popcount(am) != 1 ? (am & ~(1u << cur)) : am;
    if (!o1) o1 = am;
    int k = rnd_below(st, __builtin_popcount(o1));
    int n1 = 0;
    for (int b = 0; b < 4; b++) if (o1 & (1u << b)) { if (!k--) { n1 = b; break; } }
    const unsigned o2 = (allowed_mask[j] & 15u) & CANPAIR[n1];
    if (o2) {
      int k2 = rnd_below(st, __builtin_popcount(o2));
      for (int b = 0; b < 4; b++) if (o2 & (1u << b)) { if (!k2--) { o[pos] = LET[n1]; o[j] = LET[b]; break; } }
    }
  }
  return c.homodimer ? homodimer_copy(c, s, pos, o) : DRNA_OK;
}

// one proposal per replica; partner = partner of every design pair (target + ordinary alternative pairs), snakes optional
static int propose_impl(int R, int L, const char* target, const int32_t* partner, const unsigned char* allowed_mask,
                        const int32_t* snake_of, const int32_t* snake_off, const int32_t* snake_nodes,
                        const int32_t* snake_nstates, const char* snake_states, const char* seqs, const char* mfe_ss,
                        const int32_t* shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                        uint32_t* rng_state, char* out_seqs, int oligo_state = 0) {
  using namespace drna_host;
  ProposeCtx c;
  int rc = propose_ctx_init(c, L, target, partner, allowed_mask, snake_of, snake_off, snake_nodes, snake_nstates, snake_states,
                            n_shelves, tm_max, tm_min, targeted);
  if (rc == DRNA_OK && oligo_state) rc = propose_ctx_two_strands(c, target, oligo_state);
  if (rc != DRNA_OK) return rc;
  std::vector<int> pq(L), pool(L);
  std::vector<char> mark(L);
  for (int r = 0; r < R; r++) {
    int np = -1;
    if (targeted) {
      if (!pair_table(mfe_ss + (size_t)r * L, L, pq.data())) return DRNA_ERR_STRUCTURE;
      np = targeted_pool(c, pq.data(), mark.data(), pool.data());
    }
    rc = propose_one(c, seqs + (size_t)r * L, pool.data(), np, targeted ? shelf_probability(c, shelf_index[r]) : 0.0,
                     Mt{rng_state + (size_t)r * RNG_WORDS}, out_seqs + (size_t)r * L);
    if (rc != DRNA_OK) return rc;
  }
  return DRNA_OK;
}

extern "C" int drna_propose_batch(int R, int L, const char* target, const unsigned char* allowed_mask, const char* seqs,
                                  const char* mfe_ss, const int32_t* shelf_index, int n_shelves, double tm_max, double tm_min,
                                  int targeted, uint32_t* rng_state, char* out_seqs) {
  if (R < 0 || L < 1 || L > 2048 || !target || !allowed_mask || (R > 0 && (!seqs || !mfe_ss || !shelf_index || !rng_state || !out_seqs)))
    return DRNA_ERR_ARG;
  return propose_impl(R, L, target, nullptr, allowed_mask, nullptr, nullptr, nullptr, nullptr, nullptr, seqs, mfe_ss,
                      shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state, out_seqs);
}

extern "C" int drna_propose_batch_alt(int R, int L, const char* target, const int32_t* partner,
                                      const unsigned char* allowed_mask, const int32_t* snake_of, int n_snakes,
                                      const int32_t* snake_off, const int32_t* snake_nodes, const int32_t* snake_nstates,
                                      const char* snake_states, const char* seqs, const char* mfe_ss,
                                      const int32_t* shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                                      uint32_t* rng_state, char* out_seqs) {
  if (R < 0 || L < 1 || L > 2048 || !target || !partner || !allowed_mask || n_snakes < 0 ||
      (n_snakes > 0 && (!snake_of || !snake_off || !snake_nodes || !snake_nstates || !snake_states)) ||
      (R > 0 && (!seqs || !mfe_ss || !shelf_index || !rng_state || !out_seqs)))
    return DRNA_ERR_ARG;
  for (int k = 0; k < n_snakes; k++) {
    if (snake_off[k] < 0 || snake_off[k + 1] <= snake_off[k] || snake_nstates[k] < 1 || snake_nstates[k] > 4) return DRNA_ERR_ARG;
    for (int x = snake_off[k]; x < snake_off[k + 1]; x++)
      if (snake_nodes[x] < 0 || snake_nodes[x] >= L || snake_of[snake_nodes[x]] != k) return DRNA_ERR_ARG;
  }
  if (n_snakes > 0)
    for (int i = 0; i < L; i++)
      if (snake_of[i] >= n_snakes) return DRNA_ERR_ARG;
  return propose_impl(R, L, target, partner, allowed_mask, n_snakes ? snake_of : nullptr, snake_off, snake_nodes,
                      snake_nstates, snake_states, seqs, mfe_ss, shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state,
                      out_seqs);
}

extern "C" int drna_propose_batch_co(int R, int L, const char* target, const unsigned char* allowed_mask, int oligo_state,
                                     const char* seqs, const char* mfe_ss, const int32_t* shelf_index, int n_shelves, double tm_max,
                                     double tm_min, int targeted, uint32_t* rng_state, char* out_seqs) {
  if (R < 0 || L < 3 || L > 2048 || !target || !allowed_mask || (oligo_state != 1 && oligo_state != 2) ||
      (R > 0 && (!seqs || !mfe_ss || !shelf_index || !rng_state || !out_seqs)))
    return DRNA_ERR_ARG;
  return propose_impl(R, L, target, nullptr, allowed_mask, nullptr, nullptr, nullptr, nullptr, nullptr, seqs, mfe_ss,
                      shelf_index, n_shelves, tm_max, tm_min, targeted, rng_state, out_seqs, oligo_state);
}

extern "C" int drna_metropolis_batch(int R, const double* score_o, const double* score_m, const double* temps, double Lconst,
                                     uint32_t* rng_state, unsigned char* accept, unsigned char* better) {
  if (R < 0 || (R > 0 && (!score_o || !score_m || !temps || !rng_state || !accept || !better))) return DRNA_ERR_ARG;
  for (int r = 0; r < R; r++) {
    if (score_m[r] <= score_o[r]) { accept[r] = 1; better[r] = 1; continue; }
    better[r] = 0;
    const double p = std::exp((-Lconst / temps[r]) * (score_m[r] - score_o[r]));
    accept[r] = p > drna_host::rnd01(drna_host::Mt{rng_state + (size_t)r * drna_host::RNG_WORDS}) ? 1 : 0;   // one draw, only when the mutant is worse
  }
  return DRNA_OK;
}

// ---------------------------------------------------------------- the whole Monte-Carlo inner loop of one exchange step

// What one scoring pass over the R proposals of an iteration leaves per replica (filled by the entry point's score step)
struct McScored {
  std::vector<char> ss;                          // the chains' MFE structures, in the layout of the state strings
  std::vector<double> Epf, ed, Emfe, edef;       // kcal/mol: ensemble free energy, E(targets[0]), MFE energy; ensemble defect
  std::vector<double> add;                       // added to the -sf sum: the alternative-structure term
  std::vector<double> x0, x1;                    // two strands: oligo_fraction and the bonus, kept with an accepted state; the bonus is
                                                 // added last, after the negative-design term (the reference's order of additions)
  bool has_add = false;
};

// The chains of a loop: chain r belongs to design problem of[r] and keeps its state strings (seqs, mfe_ss: len[r] chars) at off[r].
// Problem p keeps its best strings at poff[p], its best values at best + p * best_vals and three counters.  One problem of R
// replicas (every entry point but drna_mc_run_ragged) is mc_uniform: off[r] = r * L.
struct McChains {
  int P = 1, best_vals = 0, max_len = 0;
  std::vector<int> of, len;
  std::vector<size_t> off, poff;
  size_t total = 0;
  int R() const { return (int)of.size(); }
};
static McChains mc_uniform(int R, int L) {
  McChains c;
  c.max_len = L; c.total = (size_t)R * L;
  c.of.assign(R, 0); c.len.assign(R, L); c.off.resize(R); c.poff.assign(1, 0);
  for (int r = 0; r < R; r++) c.off[r] = (size_t)r * L;
  return c;
}

// The loop every drna_mc_run* entry point runs: proposals from the chains' own streams, the entry point's scoring of all
// proposals (score_all(prop) fills S), SimScore (metrics(r, ss, pq, m): pair table of chain r's structure for the targeted
// moves, and the three rounded metrics against its target), the -sf sum, Metropolis, state update, counters and best state of
// the chain's problem (ctx[p], p < ch.P).  A chain's strings have ch.len[r] chars (two strands: with the '&'); xs0 / xs1:
// per-replica state beside the usual arrays or null.
// Negative design (sub given: the _nd entry points; utils/energy_scores.py:104-108): between scoring and Metropolis the proposals
// whose 1 - MCC is exactly 0 get their second-best fold in ONE launch (second_best(prop, hits, H) leaves E2 of hit h in
// e->hm_Emfe[h]) and lose E2 / 100 - Epf; sub[r] is the second-best energy of replica r's current state (0 where it is unsolved)
// and best[4] (two strands: best[6]) that of the best state.  So an iteration is two passes over the chains: scores of all
// proposals first, then the Metropolis draws in chain order, each from its chain's own stream as before.
// Sequence motifs (the engine's set, drna_set_motifs; utils/energy_scores.py:121-123): the term of every proposal's own string is
// the last addition of all, the same set for every problem of the loop; with an empty set nothing is searched
template <class ScoreAll, class Metrics, class SecondBest>
static int mc_loop(drna_engine* e, const char* who, const McChains& ch, int n_iter, const ProposeCtx* ctx, const int32_t* shelf_index,
                   int targeted, const double* temps, double Lconst, int n_terms, const int32_t* term_id, const double* term_w,
                   uint32_t* rng_state, char* seqs, char* mfe_ss, double* score, double* mcc1, double* Epf, double* Ed, double* xs0,
                   double* xs1, double* sub, int64_t* counters, char* best_seq, char* best_ss, double* best, McScored& S,
                   ScoreAll&& score_all, Metrics&& metrics, SecondBest&& second_best) {
  using namespace drna_host;
  const int R = ch.R();
  const size_t* off = ch.off.data();
  std::vector<char> prop(ch.total);
  std::vector<double> pscore(R), pmcc(R), p_shelf(R, 0.0), psub(sub ? R : 0);
  std::vector<unsigned char> acc(R), better(R), same(R), bad(R);
  std::vector<SimMetrics> pm(R);
  std::vector<int> hits;
  // Per chain, of its CURRENT structure: the pair table, its SimScore against the target and the targeted-move pool (what the
  // proposal compares with the target).  Parsed once here and replaced when a proposal is accepted; a proposal whose MFE
  // structure equals the current one (most single mutations of a converged replica) reuses all three
  std::vector<int> cur_pq(ch.total), prop_pq(ch.total), cur_pool(ch.total), cur_np(R, -1);
  std::vector<SimMetrics> cur_m(R);
  std::vector<char> mark(ch.max_len);
  int fail = DRNA_OK;              // the last failure; the other chains go on, as without it
  const bool with_motifs = !e->motifs.empty();
  auto refresh_pool = [&](int r) {
    if (targeted) cur_np[r] = targeted_pool(ctx[ch.of[r]], cur_pq.data() + off[r], mark.data(), cur_pool.data() + off[r]);
  };
  auto propose_all = [&] {         // the next proposal of every chain, each from its own random stream
    for (int r = 0; r < R; r++) {
      const int rc = propose_one(ctx[ch.of[r]], seqs + off[r], cur_pool.data() + off[r], cur_np[r], p_shelf[r],
                                 Mt{rng_state + (size_t)r * RNG_WORDS}, prop.data() + off[r]);
      if (rc != DRNA_OK) fail = rc;
    }
  };
  for (int r = 0; r < R; r++) {
    if (targeted) p_shelf[r] = shelf_probability(ctx[ch.of[r]], shelf_index[r]);
    if (!metrics(r, mfe_ss + off[r], cur_pq.data() + off[r], cur_m[r])) { fail = DRNA_ERR_STRUCTURE; continue; }
    refresh_pool(r);
  }
  if (n_iter > 0 && fail == DRNA_OK) propose_all();
  if (fail != DRNA_OK) { e->err = std::string(who) + ": proposal failed (unbalanced structure in the state, or a bad design problem)"; return fail; }
  static const bool mc_profile = getenv("DRNA_MC_PROFILE") != nullptr;     // diagnostics: where an iteration's host time goes (stderr)
  double prof[3] = {0, 0, 0};
  auto now_us = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; };
  for (int it = 0; it < n_iter; it++) {
    const double tp0 = mc_profile ? now_us() : 0.0;
    const int rc = score_all(prop.data());
    if (rc != DRNA_OK) return rc;
    const double tp1 = mc_profile ? now_us() : 0.0;
    hits.clear();
    for (int r = 0; r < R; r++) {
      // SimScore of the proposal's structure against the target (utils/sim_score.py:62-147)
      const int L = ch.len[r];
      same[r] = std::memcmp(S.ss.data() + off[r], mfe_ss + off[r], (size_t)L) == 0;
      SimMetrics& m = pm[r];
      m = cur_m[r];
      bad[r] = !same[r] && !metrics(r, S.ss.data() + off[r], prop_pq.data() + off[r], m);
      if (bad[r]) { fail = DRNA_ERR_STRUCTURE; continue; }
      const double ed = S.ed[r];
      // -sf terms (utils/energy_scores.py:376-398): 0 Ed-Epf, 1 1-MCC, 2 sln_Epf, 3 Ed-MFE, 4 1-precision, 5 1-recall, 6 Edef
      double tot = 0.0;
      for (int k = 0; k < n_terms; k++) {
        double v = 0.0;
        switch (term_id[k]) {
          case 0: v = ed - S.Epf[r]; break;
          case 1: v = (1 - m.mcc) * 10; break;
          case 2: v = (S.Epf[r] + 0.3759 * L + 5.7534) / 10; break;
          case 3: v = ed - S.Emfe[r]; break;
          case 4: v = (1 - m.precision) * 10; break;
          case 5: v = (1 - m.recall) * 10; break;
          case 6: v = S.edef[r]; break;
        }
        tot += v * term_w[k];
      }
      if (S.has_add) tot += S.add[r];
      pscore[r] = tot; pmcc[r] = 1 - m.mcc;
      if (sub && pmcc[r] == 0) hits.push_back(r);             // solved: the test of ReplicaScorer._negative_design, on the rounded metric
    }
    if (sub) {
      std::fill(psub.begin(), psub.end(), 0.0);
      if (!hits.empty()) {
        const int rc2 = second_best(prop.data(), hits.data(), (int)hits.size());
        if (rc2 != DRNA_OK) return rc2;
        for (size_t h = 0; h < hits.size(); h++) {
          const int r = hits[h];
          psub[r] = e->hm_Emfe[h] / 100.0;
          pscore[r] -= psub[r] - S.Epf[r];
        }
      }
    }
    for (int r = 0; r < R; r++) {
      if (bad[r]) continue;
      if (xs0) pscore[r] += S.x1[r];                          // oligomer / monomer-fraction bonus: the last addition
      const int L = ch.len[r];
      if (with_motifs) pscore[r] += motif_score(e->motifs, prop.data() + off[r], L);     // ... but for the motif term (drna_set_motifs;
                                                                                         // two strands: the string holds the '&')
      const bool same_ss = same[r];
      const SimMetrics& m = pm[r];
      int* ppq = prop_pq.data() + off[r];
      const double ed = S.ed[r];
      // Metropolis (utils/replica_exchange_monte_carlo.py:26-57): one draw from the chain's stream, only when the mutant is worse
      (void)drna_metropolis_batch(1, score + r, pscore.data() + r, temps + r, Lconst, rng_state + (size_t)r * RNG_WORDS, acc.data() + r,
                                  better.data() + r);
      if (acc[r]) {
        std::memcpy(seqs + off[r], prop.data() + off[r], (size_t)L);
        if (!same_ss) {
          std::memcpy(mfe_ss + off[r], S.ss.data() + off[r], (size_t)L);
          std::memcpy(cur_pq.data() + off[r], ppq, (size_t)L * sizeof(int));
          cur_m[r] = m;
          refresh_pool(r);
        }
        score[r] = pscore[r]; mcc1[r] = pmcc[r]; Epf[r] = S.Epf[r]; Ed[r] = ed;
        if (xs0) { xs0[r] = S.x0[r]; xs1[r] = S.x1[r]; }
        if (sub) sub[r] = psub[r];
      }
    }
    if (it + 1 < n_iter && fail == DRNA_OK) propose_all();          // the next iteration's proposals (same streams, after the Metropolis draw)
    if (fail != DRNA_OK) { e->err = std::string(who) + ": unbalanced MFE structure from the engine, or a failed proposal"; return fail; }
    const double tp2 = mc_profile ? now_us() : 0.0;
    // counters and the best state of every problem, chain by chain in chain order (first strictly better wins)
    for (int r = 0; r < R; r++) {
      const int p = ch.of[r];
      int64_t* cnt = counters + (size_t)3 * p;
      double* bst = best + (size_t)p * ch.best_vals;
      if (acc[r]) {
        cnt[0]++;
        if (better[r]) cnt[1]++;
        if (mcc1[r] < bst[0] || (mcc1[r] == bst[0] && score[r] < bst[1])) {
          bst[0] = mcc1[r]; bst[1] = score[r]; bst[2] = Epf[r]; bst[3] = Ed[r];
          if (xs0) { bst[4] = xs0[r]; bst[5] = xs1[r]; }
          if (sub) bst[xs0 ? 6 : 4] = sub[r];
          std::memcpy(best_seq + ch.poff[p], seqs + off[r], (size_t)ch.len[r]);
          std::memcpy(best_ss + ch.poff[p], mfe_ss + off[r], (size_t)ch.len[r]);
        }
      } else cnt[2]++;
    }
    if (mc_profile) { prof[0] += tp1 - tp0 - e->timing[3] * 1e3; prof[1] += tp2 - tp1; prof[2] += now_us() - tp2; }
  }
  if (mc_profile && n_iter > 0)
    fprintf(stderr, "%s: per iteration, host us: score call beyond device time %.1f, per-replica work %.1f, bookkeeping %.1f\n", who,
            prof[0] / n_iter, prof[1] / n_iter, prof[2] / n_iter);
  return DRNA_OK;
}

// the -sf term ids of the loop; sets *want_edef when the ensemble defect (term 6, utils/energy_scores.py:362-374,397-398) is among them
static int mc_terms(drna_engine* e, const char* who, int n_terms, const int32_t* term_id, bool* want_edef) {
  *want_edef = false;
  for (int k = 0; k < n_terms; k++) {
    *want_edef |= term_id[k] == 6;
    if (term_id[k] < 0 || term_id[k] > 6) { e->err = std::string(who) + ": unknown scoring term"; return DRNA_ERR_ARG; }
  }
  return DRNA_OK;
}

// drna_mc_run (subopt_e null), drna_mc_run_nd and, with oligo_frac / bonus, drna_mc_run_oa
static int mc_run_impl(drna_engine* e, const char* who, int R, int L, int n_iter, const char* target, const int32_t* partner,
                       const unsigned char* allowed_mask, const int32_t* snake_of, int n_snakes, const int32_t* snake_off,
                       const int32_t* snake_nodes, const int32_t* snake_nstates, const char* snake_states,
                       const int32_t* shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,
                       const double* temps, double Lconst, int n_terms, const int32_t* term_id, const double* term_w,
                       uint32_t flags, uint32_t* rng_state, char* seqs, char* mfe_ss, double* score, double* mcc1,
                       double* Epf, double* Ed, int64_t* counters, char* best_seq, char* best_ss, double* best, double* subopt_e,
                       double* oligo_frac = nullptr, double* bonus = nullptr) {
  using namespace drna_host;
  if (R < 1 || R > e->max_R || L < 1 || L > e->max_L || n_iter < 0 || !target || !allowed_mask || !shelf_index || !temps ||
      n_terms < 1 || !term_id || !term_w || !rng_state || !seqs || !mfe_ss || !score || !mcc1 || !Epf || !Ed || !counters ||
      !best_seq || !best_ss || !best || e->n_targets < 1 || e->L_targets != L) {
    e->err = std::string(who) + ": bad argument (targets installed with drna_set_targets for this L; every state array given)";
    return DRNA_ERR_ARG;
  }
  const int nt = e->n_targets;
  bool want_edef = false;
  { const int rc = mc_terms(e, who, n_terms, term_id, &want_edef); if (rc != DRNA_OK) return rc; }
  if (subopt_e || oligo_frac) { const int rc = fits_workspace(e, who, R); if (rc != DRNA_OK) return rc; }
  McScored S;
  S.ss.resize((size_t)R * L); S.Epf.resize(R); S.ed.resize(R); S.Emfe.resize(R);
  if (oligo_frac) { S.x0.resize(R); S.x1.resize(R); }
  if (want_edef) S.edef.resize(R);
  S.has_add = nt > 1;
  if (S.has_add) S.add.resize(R);
  std::vector<int32_t> pEmfe(R), pEd((size_t)R * nt);
  ProposeCtx ctx;
  {
    const int rc = propose_ctx_init(ctx, L, target, partner, allowed_mask, n_snakes > 0 ? snake_of : nullptr, snake_off, snake_nodes,
                                    snake_nstates, snake_states, n_shelves, tm_max, tm_min, targeted);
    if (rc != DRNA_OK) { e->err = std::string(who) + (rc == DRNA_ERR_STRUCTURE ? ": unbalanced target structure" : ": proposal failed"); return rc; }
  }
  const int* pr = ctx.pt.data();
  auto score_all = [&](const char* prop) -> int {
    int rc = drna_score_batch(e, R, L, prop, flags | DRNA_NEED_PF | DRNA_NEED_MFE | DRNA_NEED_EVAL, S.Epf.data(), pEmfe.data(),
                              S.ss.data(), pEd.data());
    if (rc != DRNA_OK) return rc;
    if (want_edef) {                        // inside + outside recursion of every proposal (fold_outside.hpp)
      rc = drna_ensemble_defect_batch(e, R, L, prop, S.edef.data(), nullptr);
      if (rc != DRNA_OK) return rc;
    }
    for (int r = 0; r < R; r++) {
      S.ed[r] = pEd[(size_t)r * nt] / 100.0;
      S.Emfe[r] = pEmfe[r] / 100.0;
      if (nt > 1) {                                           // alternative structures (:98-102)
        double sum = 0.0;
        for (int t = 1; t < nt; t++) sum += pEd[(size_t)r * nt + t] / 100.0;
        S.add[r] = sum / (nt - 1) - S.Epf[r];
      }
    }
    if (oligo_frac) {
      // -oa on (utils/energy_scores.py:118-119, :412-419): every proposal against a copy of itself, one launch now that the
      // score batch has drained; the monomer-fraction term is added by the loop, after the negative-design term
      std::memcpy(e->hm_seqs, prop, (size_t)R * L);
      rc = self_dimer_mapped(e, R, L);
      if (rc != DRNA_OK) return rc;
      for (int r = 0; r < R; r++) {
        const double* F = e->hm_F4 + (size_t)4 * r;
        S.x0[r] = oligo_fraction(F[0], F[1], F[2]);
        S.x1[r] = kT_log(1 - S.x0[r]);
      }
    }
    return DRNA_OK;
  };
  auto metrics = [&](int, const char* ss, int* pq, SimMetrics& m) {
    if (!pair_table(ss, L, pq)) return false;
    m = sim_metrics(pr, pq, L);
    return true;
  };
  auto second_best = [&](const char* prop, const int* hits, int H) -> int {
    for (int h = 0; h < H; h++) std::memcpy(e->hm_seqs + (size_t)h * L, prop + (size_t)hits[h] * L, (size_t)L);
    return second_best_mapped(e, H, L, 0);
  };
  return mc_loop(e, who, mc_uniform(R, L), n_iter, &ctx, shelf_index, targeted, temps, Lconst, n_terms, term_id, term_w, rng_state, seqs,
                 mfe_ss, score, mcc1, Epf, Ed, oligo_frac, bonus, subopt_e, counters, best_seq, best_ss, best, S, score_all, metrics,
                 second_best);
}

#define MC_RUN_PARAMS                                                                                                              \
  drna_engine *e, int R, int L, int n_iter, const char *target, const int32_t *partner, const unsigned char *allowed_mask,         \
      const int32_t *snake_of, int n_snakes, const int32_t *snake_off, const int32_t *snake_nodes, const int32_t *snake_nstates,  \
      const char *snake_states, const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted,             \
      const double *temps, double Lconst, int n_terms, const int32_t *term_id, const double *term_w, uint32_t flags,               \
      uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed, int64_t *counters,      \
      char *best_seq, char *best_ss, double *best
#define MC_RUN_ARGS                                                                                                                 \
  R, L, n_iter, target, partner, allowed_mask, snake_of, n_snakes, snake_off, snake_nodes, snake_nstates, snake_states, shelf_index, \
      n_shelves, tm_max, tm_min, targeted, temps, Lconst, n_terms, term_id, term_w, flags, rng_state, seqs, mfe_ss, score, mcc1, Epf, \
      Ed, counters, best_seq, best_ss, best

extern "C" int drna_mc_run(MC_RUN_PARAMS) {
  if (!e) return DRNA_ERR_ARG;
  return mc_run_impl(e, "drna_mc_run", MC_RUN_ARGS, nullptr);
}

extern "C" int drna_mc_run_nd(MC_RUN_PARAMS, double* subopt_e) {
  if (!e) return DRNA_ERR_ARG;
  if (!subopt_e) { e->err = "drna_mc_run_nd: bad argument (subopt_e required)"; return DRNA_ERR_ARG; }
  return mc_run_impl(e, "drna_mc_run_nd", MC_RUN_ARGS, subopt_e);
}

extern "C" int drna_mc_run_oa(MC_RUN_PARAMS, double* subopt_e, double* oligo_frac, double* bonus) {
  if (!e) return DRNA_ERR_ARG;
  if (!oligo_frac || !bonus) { e->err = "drna_mc_run_oa: bad argument (oligo_frac and bonus required)"; return DRNA_ERR_ARG; }
  return mc_run_impl(e, "drna_mc_run_oa", MC_RUN_ARGS, subopt_e, oligo_frac, bonus);
}

#define MC_RUN_CO_PARAMS                                                                                                              \
  drna_engine *e, int R, int L, int cut, int n_iter, const char *target, const unsigned char *allowed_mask, int oligo_state,          \
      const int32_t *shelf_index, int n_shelves, double tm_max, double tm_min, int targeted, const double *temps, double Lconst,      \
      int n_terms, const int32_t *term_id, const double *term_w, uint32_t *rng_state, char *seqs, char *mfe_ss, double *score,        \
      double *mcc1, double *Epf, double *Ed, double *oligo_frac, double *bonus, int64_t *counters, char *best_seq, char *best_ss,     \
      double *best
#define MC_RUN_CO_ARGS                                                                                                                \
  R, L, cut, n_iter, target, allowed_mask, oligo_state, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, Lconst, n_terms,     \
      term_id, term_w, rng_state, seqs, mfe_ss, score, mcc1, Epf, Ed, oligo_frac, bonus, counters, best_seq, best_ss, best

// drna_mc_run_cofold (subopt_e null) and drna_mc_run_cofold_nd
static int mc_run_cofold_impl(const char* who, MC_RUN_CO_PARAMS, double* subopt_e) {
  using namespace drna_host;
  const int Ls = L + 1;                      // the state strings carry the '&' at column cut
  if (R < 1 || R > e->max_R || L < 2 || L > e->max_L || n_iter < 0 || !target || !allowed_mask || !shelf_index || !temps ||
      n_terms < 1 || !term_id || !term_w || !rng_state || !seqs || !mfe_ss || !score || !mcc1 || !Epf || !Ed || !oligo_frac || !bonus ||
      !counters || !best_seq || !best_ss || !best || (oligo_state != 1 && oligo_state != 2)) {
    e->err = std::string(who) + ": bad argument (R, L within the engine's limits; oligo_state 1 or 2; every state array given)";
    return DRNA_ERR_ARG;
  }
  if (cut < 1 || cut > L - 1 || target[cut] != '&') {
    e->err = std::string(who) + ": cut outside [1, L - 1], or the target's '&' is not at column cut";
    return DRNA_ERR_ARG;
  }
  int rc = need_targets(e, who, L);
  if (rc == DRNA_OK) rc = fits_workspace(e, who, R);
  bool want_edef = false;
  if (rc == DRNA_OK) rc = mc_terms(e, who, n_terms, term_id, &want_edef);
  if (rc != DRNA_OK) return rc;
  const int nt = e->n_targets;
  McScored S;
  S.ss.resize((size_t)R * Ls); S.Epf.resize(R); S.ed.resize(R); S.Emfe.resize(R); S.x0.resize(R); S.x1.resize(R);
  if (want_edef) S.edef.resize(R);
  std::vector<char> flat(want_edef ? (size_t)R * L : 0);
  ProposeCtx ctx;
  rc = propose_ctx_init(ctx, Ls, target, nullptr, allowed_mask, nullptr, nullptr, nullptr, nullptr, nullptr, n_shelves, tm_max, tm_min,
                        targeted);
  if (rc == DRNA_OK) rc = propose_ctx_two_strands(ctx, target, oligo_state);
  if (rc != DRNA_OK || ctx.amp != cut) {
    e->err = rc == DRNA_ERR_STRUCTURE ? std::string(who) + ": unbalanced target structure" : std::string(who) + ": bad design problem";
    return rc != DRNA_OK ? rc : DRNA_ERR_ARG;
  }
  // oligomer bonus for a hetero-dimer or a homodimer of two different sub-structures, else the monomer-fraction term
  // (utils/energy_scores.py:110-118)
  const bool oligomer = oligo_state == 1 || !ctx.ss_equal;
  // SimScore with the reference's '&' -> "Ee" substitution (utils/energy_scores.py:79): the nick becomes a pair of its own in the
  // target and in every structure, so the compared strings are one longer than the state strings
  std::vector<char> xs(Ls + 1);
  std::vector<int> xr(Ls + 1), xq(Ls + 1);
  auto expand = [&](const char* ss) {
    std::memcpy(xs.data(), ss, (size_t)cut);
    xs[cut] = 'E'; xs[cut + 1] = 'e';
    std::memcpy(xs.data() + cut + 2, ss + cut + 1, (size_t)(Ls - cut - 1));
  };
  expand(target);
  if (!pair_table(xs.data(), Ls + 1, xr.data())) { e->err = std::string(who) + ": unbalanced target structure"; return DRNA_ERR_STRUCTURE; }
  auto metrics = [&](int, const char* ss, int* pq, SimMetrics& m) {
    if (ss[cut] != '&' || !pair_table(ss, Ls, pq)) return false;
    expand(ss);
    if (!pair_table(xs.data(), Ls + 1, xq.data())) return false;
    m = sim_metrics(xr.data(), xq.data(), Ls + 1);
    return true;
  };
  auto score_all = [&](const char* prop) -> int {
    for (int r = 0; r < R; r++) {             // the letters of both strands, without the '&', straight into the mapped buffer
      std::memcpy(e->hm_seqs + (size_t)r * L, prop + (size_t)r * Ls, (size_t)cut);
      std::memcpy(e->hm_seqs + (size_t)r * L + cut, prop + (size_t)r * Ls + cut + 1, (size_t)(L - cut));
    }
    if (want_edef) std::memcpy(flat.data(), e->hm_seqs, (size_t)R * L);
    int rc2 = cofold_batch_mapped(e, R, L, cut, true, true, true);
    if (rc2 != DRNA_OK) return rc2;
    for (int r = 0; r < R; r++) {
      const double* F = e->hm_F4 + (size_t)4 * r;
      S.Epf[r] = F[3];
      S.ed[r] = e->hm_Ed[(size_t)r * nt] / 100.0;
      S.Emfe[r] = e->hm_Emfe[r] / 100.0;
      char* o = S.ss.data() + (size_t)r * Ls;
      std::memcpy(o, e->hm_ss + (size_t)r * L, (size_t)cut);
      o[cut] = '&';
      std::memcpy(o + cut + 1, e->hm_ss + (size_t)r * L + cut, (size_t)(L - cut));
      S.x0[r] = oligo_fraction(F[0], F[1], F[2]);
      S.x1[r] = oligomer ? kT_log(S.x0[r]) : kT_log(1 - S.x0[r]);          // (added by the loop, after the negative-design term)
    }
    if (want_edef) {                          // inside + outside recursion under the co-fold rules (fold_cofold_outside.hpp)
      rc2 = drna_cofold_ensemble_defect_batch(e, R, L, cut, flat.data(), S.edef.data(), nullptr);
      if (rc2 != DRNA_OK) return rc2;
    }
    return DRNA_OK;
  };
  auto second_best = [&](const char* prop, const int* hits, int H) -> int {       // the letters of both strands, without the '&'
    for (int h = 0; h < H; h++) {
      const char* p = prop + (size_t)hits[h] * Ls;
      std::memcpy(e->hm_seqs + (size_t)h * L, p, (size_t)cut);
      std::memcpy(e->hm_seqs + (size_t)h * L + cut, p + cut + 1, (size_t)(L - cut));
    }
    return second_best_mapped(e, H, L, cut);
  };
  return mc_loop(e, who, mc_uniform(R, Ls), n_iter, &ctx, shelf_index, targeted, temps, Lconst, n_terms, term_id, term_w, rng_state, seqs, mfe_ss,
                 score, mcc1, Epf, Ed, oligo_frac, bonus, subopt_e, counters, best_seq, best_ss, best, S, score_all, metrics, second_best);
}

extern "C" int drna_mc_run_cofold(MC_RUN_CO_PARAMS) {
  if (!e) return DRNA_ERR_ARG;
  return mc_run_cofold_impl("drna_mc_run_cofold", e, MC_RUN_CO_ARGS, nullptr);
}

extern "C" int drna_mc_run_cofold_nd(MC_RUN_CO_PARAMS, double* subopt_e) {
  if (!e) return DRNA_ERR_ARG;
  if (!subopt_e) { e->err = "drna_mc_run_cofold_nd: bad argument (subopt_e required)"; return DRNA_ERR_ARG; }
  return mc_run_cofold_impl("drna_mc_run_cofold_nd", e, MC_RUN_CO_ARGS, subopt_e);
}

// ---------------------------------------------------------------- a set of design problems in lock-step

// drna_mc_run for P problems of different lengths: the chains of all problems make one ragged batch per iteration.  The plan of
// that batch (lengths do not change inside a call) is made once; an iteration uploads the proposals, launches, and scatters back.
// drna_mc_run_ragged_nd adds what drna_mc_run_nd adds to drna_mc_run: the ensemble defect as a scoring term (aux: one ragged
// ensemble-defect pass per iteration, planned once like the score) and the negative-design step (subopt_e given: the solved
// proposals of an iteration, whatever their puzzles, get their second-best folds in one ragged launch set).
#define MC_RAGGED_PARAMS                                                                                                           \
  drna_engine *e, int P, const int32_t *R_of, const int32_t *L_of, int n_iter, const char *targets,                                \
      const unsigned char *allowed_mask, const int32_t *shelf_index, const int32_t *n_shelves, double tm_max, double tm_min,       \
      int targeted, const double *temps, double Lconst, int n_terms, const int32_t *term_id, const double *term_w, uint32_t flags, \
      uint32_t *rng_state, char *seqs, char *mfe_ss, double *score, double *mcc1, double *Epf, double *Ed, int64_t *counters,      \
      char *best_seq, char *best_ss, double *best
#define MC_RAGGED_ARGS                                                                                                              \
  e, P, R_of, L_of, n_iter, targets, allowed_mask, shelf_index, n_shelves, tm_max, tm_min, targeted, temps, Lconst, n_terms, term_id, \
      term_w, flags, rng_state, seqs, mfe_ss, score, mcc1, Epf, Ed, counters, best_seq, best_ss, best

// aux false: drna_mc_run_ragged (term 6 refused, no negative design); true: drna_mc_run_ragged_nd
static int mc_run_ragged_impl(const char* who, MC_RAGGED_PARAMS, bool aux, double* subopt_e) {
  using namespace drna_host;
  if (!e) return DRNA_ERR_ARG;
  if (P < 1 || !R_of || !L_of || n_iter < 0 || !targets || !allowed_mask || !shelf_index || !n_shelves || !temps || n_terms < 1 ||
      !term_id || !term_w || !rng_state || !seqs || !mfe_ss || !score || !mcc1 || !Epf || !Ed || !counters || !best_seq || !best_ss ||
      !best) {
    e->err = std::string(who) + ": bad argument (P >= 1; every per-puzzle and per-chain array given)";
    return DRNA_ERR_ARG;
  }
  bool want_edef = false;
  { const int rc = mc_terms(e, who, n_terms, term_id, &want_edef); if (rc != DRNA_OK) return rc; }
  if (want_edef && !aux) { e->err = std::string(who) + ": scoring term 6 (Edef) is not available for a set of puzzles"; return DRNA_ERR_ARG; }
  McChains ch;
  ch.P = P; ch.best_vals = subopt_e ? 5 : 4; ch.poff.resize(P);
  size_t chars = 0, n_chains = 0;
  for (int p = 0; p < P; p++) {
    if (R_of[p] < 1 || L_of[p] < 1) { e->err = std::string(who) + ": puzzle " + std::to_string(p) + ": R_of < 1 or L_of < 1"; return DRNA_ERR_ARG; }
    ch.poff[p] = chars;
    chars += (size_t)L_of[p];
    n_chains += (size_t)R_of[p];
    ch.total += (size_t)R_of[p] * L_of[p];
    ch.max_len = std::max(ch.max_len, (int)L_of[p]);
  }
  if (n_chains > (size_t)e->max_R) {
    e->err = std::string(who) + ": " + std::to_string(n_chains) + " chains, more than max_R = " + std::to_string(e->max_R);
    return DRNA_ERR_ARG;
  }
  if (ch.total > (size_t)e->max_R * e->max_L) {
    e->err = std::string(who) + ": " + std::to_string(ch.total) + " nucleotides in all chains, more than max_R * max_L = " +
             std::to_string((size_t)e->max_R * e->max_L);
    return DRNA_ERR_ARG;
  }
  for (int p = 0; p < P; p++) {
    if (L_of[p] > e->max_L) { e->err = std::string(who) + ": puzzle " + std::to_string(p) + ": L_of above max_L"; return DRNA_ERR_ARG; }
    for (int i = 0; i < L_of[p]; i++) {
      const char c = targets[ch.poff[p] + i];
      if (c != '(' && c != ')' && c != '.') {
        e->err = std::string(who) + ": puzzle " + std::to_string(p) + ": target holds '" + c + "' (one strand and the plain brackets ( ) . only)";
        return DRNA_ERR_ARG;
      }
    }
  }
  const int C = (int)n_chains;
  if (subopt_e) { const int rc = fits_workspace(e, who, C); if (rc != DRNA_OK) return rc; }
  std::vector<ProposeCtx> ctx(P);
  std::vector<int32_t> lens(C);
  ch.of.resize(C); ch.len.resize(C); ch.off.resize(C);
  {
    size_t o = 0;
    int r = 0;
    for (int p = 0; p < P; p++) {
      const int rc = propose_ctx_init(ctx[p], L_of[p], targets + ch.poff[p], nullptr, allowed_mask + ch.poff[p], nullptr, nullptr,
                                      nullptr, nullptr, nullptr, n_shelves[p], tm_max, tm_min, targeted);
      if (rc != DRNA_OK) {
        e->err = std::string(who) + ": puzzle " + std::to_string(p) + (rc == DRNA_ERR_STRUCTURE ? ": unbalanced target structure" : ": proposal failed");
        return rc;
      }
      for (int k = 0; k < R_of[p]; k++, r++) {
        ch.of[r] = p; ch.len[r] = lens[r] = L_of[p]; ch.off[r] = o;
        o += (size_t)L_of[p];
      }
    }
  }
  // the call's own targets: a set left from an earlier call (more puzzles, other structures) must not be evaluated against
  { const int rc = drna_set_targets_ragged(e, P, L_of, targets); if (rc != DRNA_OK) return rc; }
  RaggedPlan plan;
  { const int rc = ragged_plan(e, C, lens.data(), ch.of.data(), flags | DRNA_NEED_PF | DRNA_NEED_MFE | DRNA_NEED_EVAL, plan); if (rc != DRNA_OK) return rc; }
  RaggedPlan edef_plan;
  if (want_edef) { const int rc = edef_ragged_plan(e, who, C, lens.data(), ch.of.data(), edef_plan); if (rc != DRNA_OK) return rc; }
  McScored S;
  S.ss.resize(ch.total); S.Epf.resize(C); S.ed.resize(C); S.Emfe.resize(C);
  if (want_edef) S.edef.resize(C);
  std::vector<int32_t> pEmfe(C), pEd(C), hit_len(subopt_e ? C : 0);
  auto score_all = [&](const char* prop) -> int {
    int rc = ragged_run(e, plan, prop, S.Epf.data(), pEmfe.data(), S.ss.data(), pEd.data());
    if (rc != DRNA_OK) return rc;
    if (want_edef) {                        // inside + outside recursion of every proposal of every puzzle
      rc = edef_ragged_run(e, edef_plan, prop, S.edef.data());
      if (rc != DRNA_OK) return rc;
    }
    for (int r = 0; r < C; r++) { S.ed[r] = pEd[r] / 100.0; S.Emfe[r] = pEmfe[r] / 100.0; }
    return DRNA_OK;
  };
  auto metrics = [&](int r, const char* ss, int* pq, SimMetrics& m) {
    if (!pair_table(ss, ch.len[r], pq)) return false;
    m = sim_metrics(ctx[ch.of[r]].pt.data(), pq, ch.len[r]);
    return true;
  };
  // the solved proposals, whatever their puzzles, one after the other in the staging buffer: E2 of hit h comes back in hm_Emfe[h]
  auto second_best = [&](const char* prop, const int* hits, int H) -> int {
    size_t o = 0;
    for (int k = 0; k < H; k++) {
      const int r = hits[k];
      hit_len[k] = ch.len[r];
      std::memcpy(e->hm_seqs + o, prop + ch.off[r], (size_t)ch.len[r]);
      o += (size_t)ch.len[r];
    }
    return second_best_ragged(e, H, hit_len.data(), e->dm_seqs, e->dm_Emfe, nullptr);
  };
  return mc_loop(e, who, ch, n_iter, ctx.data(), shelf_index, targeted, temps, Lconst, n_terms, term_id, term_w, rng_state, seqs,
                 mfe_ss, score, mcc1, Epf, Ed, nullptr, nullptr, subopt_e, counters, best_seq, best_ss, best, S, score_all, metrics,
                 second_best);
}

extern "C" int drna_mc_run_ragged(MC_RAGGED_PARAMS) { return mc_run_ragged_impl("drna_mc_run_ragged", MC_RAGGED_ARGS, false, nullptr); }

extern "C" int drna_mc_run_ragged_nd(MC_RAGGED_PARAMS, double* subopt_e) {
  return mc_run_ragged_impl("drna_mc_run_ragged_nd", MC_RAGGED_ARGS, true, subopt_e);
}

// ---------------------------------------------------------------- option "poison" (tests)

// Option "poison" (tests): every scratch buffer that exists right now filled with one byte, the streams drained before and after.
// Scratch is what every call writes before it reads (the table of buffers): the workspaces, the result and staging
// buffers, the status words, the exchange rows and records, the ragged descriptors and the masks.  State stays as it is: the
// parameter tables and plans, installed targets (d_pt, d_rpt, d_rpt_off), the all-unpaired table d_mea_pt (written once), the
// motifs, and the three sets of hand-over flags, whose epoch rule is their own protocol (a poisoned flag is a wait that never ends).
static int poison_scratch(drna_engine* e, int byte) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const int ld = e->max_L + 2;
  const size_t R = (size_t)e->max_R, L = (size_t)e->max_L, slots = (size_t)e->ws_slots;
  const size_t kb_stride = (size_t)3 * 8 * ld * ld + (size_t)cofold_kbest_ws_extra(8, ld);        // (ranked_structs_batch)
  const size_t xrows = (size_t)2 * (MFE_FAST_NMAX + 2) * XP;                                      // (prepare_folds)
  const struct { void* p; size_t bytes; } dev[] = {
      {e->d_ws_mfe, mfe_ws_stride(ld) * sizeof(int32_t) * slots},
      {e->d_ws_pf, pf_ws_stride(ld) * sizeof(double) * slots},
      {e->d_ws_out, (size_t)outside_ws_stride(ld) * sizeof(double) * slots},
      {e->d_ws_kb, kb_stride * sizeof(int32_t) * e->kb_chunk},
      {e->d_kbE, (size_t)8 * e->kb_chunk * sizeof(int32_t)},
      {e->d_kbss, (size_t)8 * e->kb_chunk * L},
      {e->d_q5s, slots * ld * sizeof(double)},
      {e->d_cocols, slots * CO_COLS * ld * sizeof(double)},
      {e->d_seqs, R * L},
      {e->d_ss, R * L},
      {e->d_Epf, R * sizeof(double)},
      {e->d_Emfe, R * sizeof(int32_t)},
      {e->d_Ed, R * std::max(1, e->n_targets) * sizeof(int32_t)},
      {e->d_edef, R * sizeof(double)},
      {e->d_F4, 4 * R * sizeof(double)},
      {e->d_xs, (size_t)e->dual_cap * 256 * sizeof(int32_t)},
      {e->d_xa_mfe, (size_t)e->dual_cap * xrows * sizeof(int32_t)},
      {e->d_xb_mfe, (size_t)e->dual_cap * xrows * sizeof(int32_t)},
      {e->d_srec, (size_t)e->srec_stride * R * sizeof(int32_t)},
      {e->d_rg, (size_t)RG_BLOCKS * 7 * R * sizeof(int)},
      {e->d_nopair, e->nopair_cap},
  };
  for (const auto& b : dev)
    if (b.p && b.bytes) HIP_TRY(hipMemset(b.p, byte, b.bytes));
  HIP_TRY(hipDeviceSynchronize());        // (the memsets run on the null stream, the kernels on non-blocking streams of their own)
  // host-mapped: the status words, the staging buffers and the fused launch's clocks
  const struct { void* p; size_t bytes; } host[] = {
      {e->h_status, 2 * R * sizeof(int32_t)},
      {e->hm_seqs, R * L},
      {e->hm_ss, R * L},
      {e->hm_Epf, R * sizeof(double)},
      {e->hm_Emfe, R * sizeof(int32_t)},
      {e->hm_Ed, e->hm_Ed_cap * sizeof(int32_t)},
      {e->hm_F4, 4 * R * sizeof(double)},
      {e->h_clk, (size_t)2 * e->clk_cap * sizeof(long long)},
  };
  for (const auto& b : host)
    if (b.p && b.bytes) memset(b.p, byte, b.bytes);
  return DRNA_OK;
}
