// fold_cofold_sample.hpp -- stochastic traceback for two strands: co-fold structures drawn from the ensemble of drna_cofold_batch
// and drna_cofold_ensemble_defect_batch on gfx950.  A structure of the concatenation weighs its Boltzmann factor,
// times kappa if a pair joins the strands (kappa = expDuplexInit, halved for two equal strands); the weights sum to exp(-FAB / kT).
// Runs after cofold_pf_kernel (fold_cofold.hpp) on the tables that kernel left in the workspace slot (QB, QM, QM1 of ld^2 doubles,
// the INFO bytes behind them; diagonal-major) -- always the workspace instance, the LDS instance leaves no tables.
//
// THE COLUMNS.  cofold_pf_kernel keeps q5, qA3 and qB5 in LDS, gone when it ends.  cofold_columns_kernel (one workgroup per pair,
// waves side by side, as cofold_outside_kernel does it) rebuilds them from the finished tables with that kernel's own steps
// (co_qA3_step, co_qB5_step, co_q5_column) and adds q5c, the connected part of q5 (co_q5c_column, fold_cofold.hpp), into a buffer
// of four columns per pair.  co_pf_finish forms the connected part as q5[n] - QA QB; a sampler cannot draw from a difference, and
// where the connected share is 1e-6 the difference has lost its digits.  ROOT therefore draws against QA QB + kappa q5c[n], which
// differs from the fill's Q by rounding only.
//
// ONE WAVE PER SAMPLE, R x G workgroups, as sample_kernel (fold_sample.hpp), whose wave-level pick (sample_chunk) and random
// numbers (sample_rng.hpp) are used as they are.  A sample is a walk over segments on a small stack in LDS that every lane pushes
// and pops alike; the candidates of a segment are the summands of cofold_pf_body's recurrences, term for term:
//   ROOT           QA QB + kappa q5c[n]     unconnected: EXTA [1..cut] + EXTB [cut+1..n];  connected: EXTC [1..n]
//   EXTA [x..cut]  qA3[x]   = qA3[x+1] scale + sum_k stem(x,k) qA3[k+1]
//   EXTB [cut+1..y] qB5[y]  = qB5[y-1] scale + sum_k qB5[k-1] stem(k,y)
//   EXT5 [1..j], j <= cut   q5[j]  = q5[j-1] scale + sum_i q5[i-1] stem(i,j)
//   EXTC [1..j], j > cut    q5c[j] = q5c[j-1] scale + sum_{cut<i<j} q5c[i-1] stem(i,j)  (EXTC left of a pair inside strand B)
//                                                   + sum_{i<=cut} q5[i-1] stem(i,j)    (EXT5 left of THE joining pair)
//   PAIR (i,j)     qb[i,j]  = hairpin (same strand) | qA3[i+1] qB5[j-1] x nick loop (joining pair: EXTA + EXTB inside it)
//                             + sum over the 496 loop shapes (both stretches inside a strand, inner pair at dp >= 1)
//                             + multiloop closing x sum_k qm[i+1,k-1] qm1[k,j-1]  (i ~ i+1, j-1 ~ j, k-1 ~ k)
//   QM   [i,j]     qm[i,j]  = qm1[i,j] + sum_k expMLbase^(k-i) qm1[k,j] (i..k on one strand) + sum_k qm[i,k-1] qm1[k,j] (k-1 ~ k)
//   QM1  [i,j]     qm1[i,j] = sum_l qb[i,l] MLstem(i,l) expMLbase^(j-l)  while no nick lies between l and j
// (x ~ y: neighbours on one strand).  A step is wave-uniform: threshold u x (table value), candidates over the lanes in chunks of
// 64 in a fixed order, prefix sum and ballot, the LAST candidate of non-zero weight as the fallback against rounding.
//
// BOUNDS.  A segment that can only be all-unpaired (EXTA / EXTB / EXT5 shorter than TURN + 2) is not pushed.  A joining PAIR may
// enclose nothing (i = cut, j = cut + 1).  Pending segments are disjoint; those that do not enclose the nick hold at least TURN + 2
// nucleotides and at most ONE encloses it, so the stack never holds more than n / (TURN + 2) + 1 words before the two pushes of a
// step: CO_SAMPLE_STACK = MAXN / 4 + 8.  Steps: ROOT, at most n exterior steps (each leaves a base unpaired or makes a pair), n / 2
// PAIR, n / 2 QM1 and n QM steps (one per stem of a multiloop, one per split): fewer than 4 n + 8.  On either bound the walk ends
// as the one-strand walk does (break, string as built).
//
// Random numbers: u(seed_r, s, k), k = index of the step within the sample (ROOT is step 0, every popped segment draws once) --
// sample s of a pair depends on the two sequences, the pair's seed and s alone.  Output per sample: n bytes of ( ) . over the
// concatenation (no '&') and, with E, the energy by eval_structure.hpp's loop sum with the nick (DuplexInit for a connected
// structure).  A pair whose cofold_pf_kernel status is not OK writes nothing (the host reports it).
#pragma once
#include "eval_structure.hpp"
#include "fold_cofold.hpp"
#include "fold_sample.hpp"
#include "sample_rng.hpp"

namespace drna {

constexpr int CO_SAMPLE_STACK = MAXN / 4 + 8;
enum : int { CG_ROOT = 0, CG_EXTA = 1, CG_EXTB = 2, CG_EXT5 = 3, CG_EXTC = 4, CG_PAIR = 5, CG_QM = 6, CG_QM1 = 7 };
enum : int { CO_COL_Q5 = 0, CO_COL_QA3 = 1, CO_COL_QB5 = 2, CO_COL_Q5C = 3, CO_COLS = 4 };

struct CoSampleArgs {
  CoArgs co;                    // what cofold_pf_kernel was launched with: tables, letters, L, cut, ld, workspace, status words
  EvalArgs ev;                  // T, hp_len, bulge_len, int_len, cut, DuplexInit
  double* cols;                 // per pair: q5, qA3, qB5, q5c, col_stride doubles each (cofold_columns_kernel writes them)
  long long col_stride;         // >= L + 2
  const uint64_t* seeds;        // R
  int S;                        // samples per pair
  int G;                        // workgroups per pair
  char* ss;                     // R x S x L
  int32_t* E;                   // R x S (dcal/mol) or null
};

// ---------------------------------------------------------------- the columns

struct CoColSmem : CoPfSmemCore<MAXN> {
  double q5c[MAXN + 2];
};

template <int NT>
__global__ __launch_bounds__(NT) void cofold_columns_kernel(CoSampleArgs A) {
  constexpr int NW = NT / WAVE;
  __shared__ CoColSmem sm;
  const CoArgs& C = A.co;
  const int r = blockIdx.x;
  const int n = C.L, cut = C.cut;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  if (C.status_pf[r] != ST_OK) return;    // bad character / PF out of range: nothing to rebuild (the whole workgroup leaves)
  const CoSquare lay{n, cut, C.ld};
  const PfTables& T = *C.F;
  const double* QB = C.wsp + (long long)r * C.wsp_stride;
  const unsigned char* INFO = reinterpret_cast<const unsigned char*>(QB + 3ll * C.ld * C.ld);
  const double sc1 = C.scale[1];

  stage_energy_tables<NT>(sm, T, tid);
  for (int k = tid; k <= n + 2; k += NT) {               // as cofold_pf_body starts them
    sm.qA3[k] = k == cut ? sc1 : 1.0;
    sm.qB5[k] = k == cut + 1 && k <= n ? sc1 : 1.0;
  }
  lay.template load<NT>(sm, C.seqs, r, tid);
  if (wave == 0)
    for (int x = cut - 1; x >= 1; x--) co_qA3_step(sm, lay, QB, INFO, x, T.TermAU, sc1, lane);
  if (wave == 1 % NW)
    for (int y = cut + 2; y <= n; y++) co_qB5_step(sm, lay, QB, INFO, y, T.TermAU, sc1, lane);
  if (wave == 2 % NW) co_q5_column(sm, lay, QB, INFO, T.TermAU, sc1, lane);
  __syncthreads();
  if (wave == 3 % NW) co_q5c_column(sm, lay, QB, INFO, T.TermAU, sc1, lane);
  __syncthreads();
  double* out = A.cols + (long long)r * CO_COLS * A.col_stride;
  for (int k = tid; k <= n + 1; k += NT) {
    out[CO_COL_Q5 * A.col_stride + k] = k <= n ? sm.q5[k] : 0.0;
    out[CO_COL_QA3 * A.col_stride + k] = sm.qA3[k];
    out[CO_COL_QB5 * A.col_stride + k] = sm.qB5[k];
    out[CO_COL_Q5C * A.col_stride + k] = k <= n ? sm.q5c[k] : 0.0;
  }
}

// ---------------------------------------------------------------- the walk

struct CoSampleWaveSmem {
  EvalSmem ev;                  // codes and the pair table of the sample being drawn
  int seg[CO_SAMPLE_STACK];     // kind | i << 3 | j << 15
};
template <int NW>
struct CoSampleSmem {
  double stack[64];
  double mmH[128], mmI[128], mm1n[128], mm23[128], mmM[128], mmExt[128];
  double int11[1024];
  double d5[32], d3[32];
  int plan_u[NPLAN];            // u1 | u2 << 8 (the fill's order)
  unsigned char S[MAXN + 4];
  int flag;
  CoSampleWaveSmem w[NW];
};

// the tables and columns of one pair as the walk reads them
struct CoSampleTabs {
  const double *QB, *QM, *QM1, *q5, *qA3, *qB5, *q5c;
  const unsigned char* INFO;
  int n, cut, ld;
  double sc1, sc2, kap;         // kap: eDuplexInit, halved for two equal strands
};

// qb[i,j] x the exterior-stem factor of the pair (i,j), i < j; 0 when the cell holds no pair (co_q5_column's term without its prefix)
template <class SM>
__device__ __forceinline__ double cosample_stem(const SM& sm, const CoSampleTabs& X, double tAU, int i, int j, bool h5, bool h3) {
  const int c = (j - i) * X.ld + i;
  const int fi = X.INFO[c];
  if (!fi) return 0.0;
  const int t = rtype_of(fi >> 4);
  return X.QB[c] * (t > 2 ? tAU : 1.0) * co_pf_endstem(sm.mmExt, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
}

// candidate c of an exterior segment: 0 = the open end unpaired, else a pair at the open end
//   EXTA [x..cut]:   c = k - x, the pair (x, k)       EXTB [cut+1..y]: c = k - cut, the pair (k, y)
//   EXT5 / EXTC [1..j]: c = i, the pair (i, j)
__device__ __forceinline__ int cosample_ext_count(const CoSampleTabs& X, int kind, int i, int j) {
  return kind == CG_EXTA ? X.cut - i + 1 : kind == CG_EXTB ? j - X.cut : j;
}
template <class SM>
__device__ __forceinline__ double cosample_ext_weight(const SM& sm, const CoSampleTabs& X, double tAU, int kind, int i, int j, int c) {
  const int n = X.n, cut = X.cut;
  if (kind == CG_EXTA) {
    if (c == 0) return X.qA3[i + 1] * X.sc1;
    const int k = i + c;
    return cosample_stem(sm, X, tAU, i, k, i > 1, k < cut) * X.qA3[k + 1];
  }
  if (kind == CG_EXTB) {
    if (c == 0) return X.qB5[j - 1] * X.sc1;
    const int k = cut + c;
    return X.qB5[k - 1] * cosample_stem(sm, X, tAU, k, j, k > cut + 1, j < n);
  }
  const bool h5 = c > 1 && co_same(c - 1, c, cut), h3 = j < n && co_same(j, j + 1, cut);
  if (kind == CG_EXT5) {
    if (c == 0) return X.q5[j - 1] * X.sc1;
    return X.q5[c - 1] * cosample_stem(sm, X, tAU, c, j, h5, h3);
  }
  if (c == 0) return X.q5c[j - 1] * X.sc1;
  return (c <= cut ? X.q5[c - 1] : X.q5c[c - 1]) * cosample_stem(sm, X, tAU, c, j, h5, h3);
}

// candidate c of PAIR (i,j): 0 = hairpin (same strand) or the loop with the nick (joining pair), 1 + e = entry e of the loop plan,
// 1 + NPLAN + m = multiloop split at k = i + 3 + m: qm[i+1, k-1], qm1[k, j-1]
__device__ __forceinline__ int cosample_pair_count(int d) { return 1 + NPLAN + (d - 4 > 0 ? d - 4 : 0); }
template <class SM>
__device__ __forceinline__ double cosample_pair_weight(const SM& sm, const CoArgs& A, const PfArgs& H, const CoSampleTabs& X, int i, int j, int c) {
  const PfTables& T = *A.F;
  const int d = j - i, ld = X.ld, cut = X.cut;
  const int t = pair_type(sm.S[i], sm.S[j]);
  if (!t) return 0.0;
  const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
  const double tau = t > 2 ? T.TermAU : 1.0;
  const bool adj_i = co_same(i, i + 1, cut), adj_j = co_same(j - 1, j, cut);
  if (c == 0) {
    if (co_same(i, j, cut)) return d > TURN ? pf_hairpin(sm, H, i, j, t) : 0.0;
    return X.qA3[i + 1] * X.qB5[j - 1] * X.sc2 * tau * co_pf_endstem(sm.mmExt, sm, rtype_of(t), adj_j, sj1, adj_i, si1);
  }
  if (c <= NPLAN) {
    const int pu = sm.plan_u[c - 1];
    const int u1 = pu & 255, u2 = pu >> 8;
    const int dp = d - 2 - u1 - u2;
    if (dp < 1) return 0.0;
    const int p = i + 1 + u1, q = j - 1 - u2;
    if (!co_same(i, p, cut) || !co_same(q, j, cut)) return 0.0;
    const int at = dp * ld + p;
    const int fi = X.INFO[at];
    if (!fi) return 0.0;
    return X.QB[at] * co_pf_intloop(sm, T, A.scale, u1, u2, t, si1, sj1, fi);
  }
  const int k = i + 3 + (c - NPLAN - 1);
  if (!(adj_i && adj_j) || k > j - 2 || k - 1 == cut) return 0.0;
  return X.QM[(k - i - 2) * ld + i + 1] * X.QM1[(j - 1 - k) * ld + k] *
         (T.MLclosing * T.MLintern * tau * sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1] * X.sc2);
}

// candidate c of QM [i,j], d = j - i: 0 = qm1[i,j]; 1 .. d-1 = unpaired prefix, qm1[i+c, j]; d .. 2d-2 = the split at
// k = i + c - d + 1: qm[i, k-1] qm1[k, j]
__device__ __forceinline__ int cosample_qm_count(int d) { return 2 * d - 1; }
__device__ __forceinline__ double cosample_qm_weight(const CoArgs& A, const CoSampleTabs& X, int i, int j, int c) {
  const int d = j - i, ld = X.ld, cut = X.cut;
  if (c == 0) return X.QM1[d * ld + i];
  if (c < d) {
    const int k = i + c;
    return co_same(i, k, cut) ? A.eMLb[c] * X.QM1[(j - k) * ld + k] : 0.0;
  }
  const int k = i + c - d + 1;
  if (k < i + 2 || k - 1 == cut) return 0.0;              // (k = i + 1: the empty segment on the left)
  return X.QM[(k - 1 - i) * ld + i] * X.QM1[(j - k) * ld + k];
}

// candidate c of QM1 [i,j]: the pair (i, j - c), c unpaired bases behind it on the pair's strand
__device__ __forceinline__ int cosample_qm1_count(int d) { return d; }
template <class SM>
__device__ __forceinline__ double cosample_qm1_weight(const SM& sm, const CoArgs& A, const CoSampleTabs& X, int i, int j, int c) {
  const PfTables& T = *A.F;
  const int n = X.n, cut = X.cut;
  const int l = j - c;
  if (!co_same(l, j, cut)) return 0.0;                    // a nick between l and j
  const int at = (l - i) * X.ld + i;
  const int fi = X.INFO[at];
  if (!fi) return 0.0;
  const int t = rtype_of(fi >> 4);
  const bool h5 = i > 1 && co_same(i - 1, i, cut), h3 = l < n && co_same(l, l + 1, cut);
  const double w = X.QB[at] * T.MLintern * (t > 2 ? T.TermAU : 1.0) * co_pf_endstem(sm.mmM, sm, t, h5, sm.S[i - 1], h3, sm.S[l + 1]);
  return c ? w * A.eMLb[c] : w;
}

__device__ __forceinline__ int cosample_seg(int kind, int i, int j) { return kind | (i << 3) | (j << 15); }

// one sample by one wave: the pair table ends in W.ev.pt
template <class SM>
__device__ __forceinline__ void cosample_walk(const SM& sm, CoSampleWaveSmem& W, const CoArgs& A, const PfArgs& H, const CoSampleTabs& X,
                                              uint64_t key, int lane) {
  const int n = X.n, ld = X.ld, cut = X.cut;
  const double tAU = A.F->TermAU;
  for (int x = lane; x < n + 2; x += WAVE) W.ev.pt[x] = 0;
  wave_lds_sync();
  // every lane pushes and pops the same words: a lane reads back what it has stored itself, no rendezvous needed
  int sp = 0;
  W.seg[sp++] = cosample_seg(CG_ROOT, 1, n);
  for (int step = 0; sp > 0 && step < 4 * n + 8; step++) {
    const int word = __builtin_amdgcn_readfirstlane(W.seg[--sp]);
    const int kind = word & 7, i = (word >> 3) & 4095, j = word >> 15;
    const int d = j - i;
    int N;
    double tabv;
    if (kind == CG_ROOT) { N = 2; tabv = X.qA3[1] * X.qB5[n] + X.kap * X.q5c[n]; }
    else if (kind == CG_EXTA) { N = cosample_ext_count(X, kind, i, j); tabv = X.qA3[i]; }
    else if (kind == CG_EXTB) { N = cosample_ext_count(X, kind, i, j); tabv = X.qB5[j]; }
    else if (kind == CG_EXT5) { N = cosample_ext_count(X, kind, i, j); tabv = X.q5[j]; }
    else if (kind == CG_EXTC) { N = cosample_ext_count(X, kind, i, j); tabv = X.q5c[j]; }
    else if (kind == CG_PAIR) { N = cosample_pair_count(d); tabv = X.QB[d * ld + i]; }
    else if (kind == CG_QM) { N = cosample_qm_count(d); tabv = X.QM[d * ld + i]; }
    else { N = cosample_qm1_count(d); tabv = X.QM1[d * ld + i]; }
    if (kind == CG_PAIR && lane == 0) { W.ev.pt[i] = (short)j; W.ev.pt[j] = (short)i; }
    SamplePick p{sample_u_key(key, (uint64_t)step) * tabv, 0.0, -1, -1};
    for (int c0 = 0; c0 < N; c0 += WAVE) {
      const int c = c0 + lane;
      double w = 0.0;
      if (c < N) {
        if (kind == CG_ROOT) w = c == 0 ? X.qA3[1] * X.qB5[n] : X.kap * X.q5c[n];
        else if (kind <= CG_EXTC) w = cosample_ext_weight(sm, X, tAU, kind, i, j, c);
        else if (kind == CG_PAIR) w = cosample_pair_weight(sm, A, H, X, i, j, c);
        else if (kind == CG_QM) w = cosample_qm_weight(A, X, i, j, c);
        else w = cosample_qm1_weight(sm, A, X, i, j, c);
      }
      if (sample_chunk(p, w, c0, lane)) break;
    }
    const int c = p.chosen >= 0 ? p.chosen : p.last;
    if (c < 0 || sp + 2 > CO_SAMPLE_STACK) break;           // (no candidate of non-zero weight: tables the fill did not leave)
    if (kind == CG_ROOT) {
      if (c == 0) {
        if (cut > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTA, 1, cut);
        if (n - cut > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTB, cut + 1, n);
      } else W.seg[sp++] = cosample_seg(CG_EXTC, 1, n);
    } else if (kind == CG_EXTA) {
      const int x = c == 0 ? i + 1 : i + c + 1;             // what is left: [x..cut]
      if (cut - x + 1 > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTA, x, cut);
      if (c) W.seg[sp++] = cosample_seg(CG_PAIR, i, i + c);
    } else if (kind == CG_EXTB) {
      const int y = c == 0 ? j - 1 : cut + c - 1;           // what is left: [cut+1..y]
      if (y - cut > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTB, cut + 1, y);
      if (c) W.seg[sp++] = cosample_seg(CG_PAIR, cut + c, j);
    } else if (kind == CG_EXT5) {
      const int rest = c == 0 ? j - 1 : c - 1;
      if (rest > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXT5, 1, rest);
      if (c) W.seg[sp++] = cosample_seg(CG_PAIR, c, j);
    } else if (kind == CG_EXTC) {
      const int rest = c == 0 ? j - 1 : c - 1;
      if (c == 0 || c > cut) { if (rest > cut) W.seg[sp++] = cosample_seg(CG_EXTC, 1, rest); }
      else if (rest > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXT5, 1, rest);
      if (c) W.seg[sp++] = cosample_seg(CG_PAIR, c, j);
    } else if (kind == CG_PAIR) {
      if (c == 0) {
        if (co_same(i, j, cut)) continue;                   // hairpin
        if (cut - i > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTA, i + 1, cut);
        if (j - 1 - cut > TURN + 1) W.seg[sp++] = cosample_seg(CG_EXTB, cut + 1, j - 1);
      } else if (c <= NPLAN) {
        const int pu = sm.plan_u[c - 1];
        W.seg[sp++] = cosample_seg(CG_PAIR, i + 1 + (pu & 255), j - 1 - (pu >> 8));
      } else {
        const int k = i + 3 + (c - NPLAN - 1);
        W.seg[sp++] = cosample_seg(CG_QM, i + 1, k - 1);
        W.seg[sp++] = cosample_seg(CG_QM1, k, j - 1);
      }
    } else if (kind == CG_QM) {
      if (c < d) W.seg[sp++] = cosample_seg(CG_QM1, i + c, j);
      else {
        const int k = i + c - d + 1;
        W.seg[sp++] = cosample_seg(CG_QM, i, k - 1);
        W.seg[sp++] = cosample_seg(CG_QM1, k, j);
      }
    } else {
      W.seg[sp++] = cosample_seg(CG_PAIR, i, j - c);
    }
  }
  wave_lds_sync();
}

template <int NT>
__global__ __launch_bounds__(NT) void cofold_sample_kernel(CoSampleArgs A) {
  constexpr int NW = NT / WAVE;
  __shared__ CoSampleSmem<NW> sm;
  const CoArgs& C = A.co;
  const int G = A.G;
  const int r = blockIdx.x / G, g = blockIdx.x - r * G;
  const int n = C.L, ld = C.ld, cut = C.cut;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());

  stage_energy_tables<NT>(sm, *C.F, tid);
  for (int e = tid; e < NPLAN; e += NT) sm.plan_u[e] = C.plan->tb_u1[e] | (C.plan->tb_u2[e] << 8);
  load_sequence<NT>(sm, C.seqs + (long long)r * n, n, tid);
  if (C.status_pf[r] != ST_OK) return;    // bad character / PF out of range: the host reports it

  PfArgs H;                               // for pf_hairpin()
  H.T = C.F; H.plan = C.plan; H.hp_w = C.hp_w; H.scale = C.scale; H.eMLb = C.eMLb; H.seqs = C.seqs; H.L = n; H.ld = 0;
  H.ws = nullptr; H.ws_stride = 0; H.Epf = nullptr; H.status = nullptr;

  const double* base = C.wsp + (long long)r * C.wsp_stride;
  const long long tab = (long long)ld * ld;
  const double* col = A.cols + (long long)r * CO_COLS * A.col_stride;
  CoSampleTabs X;
  X.QB = base; X.QM = base + tab; X.QM1 = base + 2 * tab;
  X.INFO = reinterpret_cast<const unsigned char*>(base + 3 * tab);
  X.q5 = col + CO_COL_Q5 * A.col_stride; X.qA3 = col + CO_COL_QA3 * A.col_stride;
  X.qB5 = col + CO_COL_QB5 * A.col_stride; X.q5c = col + CO_COL_Q5C * A.col_stride;
  X.n = n; X.cut = cut; X.ld = ld;
  X.sc1 = C.scale[1]; X.sc2 = C.scale[2];
  X.kap = co_homodimer(sm, n, cut) ? 0.5 * C.eDuplexInit : C.eDuplexInit;     // rotational symmetry of a homodimer

  CoSampleWaveSmem& W = sm.w[wave];
  for (int x = lane; x < n + 2; x += WAVE) W.ev.S[x] = sm.S[x];
  const uint64_t seed = A.seeds[r];
  for (int s = g * NW + wave; s < A.S; s += G * NW) {
    cosample_walk(sm, W, C, H, X, sample_key(seed, (uint64_t)s), lane);
    char* out = A.ss + ((long long)r * A.S + s) * n;
    for (int x = lane; x < n; x += WAVE) {
      const int q = W.ev.pt[x + 1];
      out[x] = q == 0 ? '.' : q > x + 1 ? '(' : ')';
    }
    if (A.E) {
      const int e = eval_loaded(W.ev, A.ev, n, lane);
      if (lane == 0) A.E[(long long)r * A.S + s] = e;
    }
    wave_lds_sync();                      // the next sample clears the pair table
  }
}

}  // namespace drna
